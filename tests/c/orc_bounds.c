/* orc_bounds.c -- the CPU restatement (oracle/restate) under AddressSanitizer.
 *
 * Built by tests/test_sanitize.py with  gcc -fsanitize=address,undefined  together with oracle/restate/*.c.  The
 * restatement gives every activation tensor a buffer of its own with slack behind it; the reference's byte-wise
 * layers reach past their tensors' ends into that slack.  With too little slack a layer must stop with ORC_E_BOUNDS
 * before it touches anything outside an allocation, so no graph may trip the sanitizer at any slack.
 *
 *   orc_bounds <slack_mult> model.mars input.bin [model.mars input.bin ...]
 * Prints one line per graph, "rc <code>"; exit code 0 unless a file cannot be read or opened.
 */
#include <stdio.h>
#include <stdlib.h>

#include "orc.h"

static void *slurp(const char *path, size_t *n) {
    FILE *f = fopen(path, "rb");
    if (!f) return NULL;
    fseek(f, 0, SEEK_END);
    const long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    void *buf = malloc(sz > 0 ? (size_t)sz : 1);
    *n = sz > 0 && fread(buf, 1, (size_t)sz, f) == (size_t)sz ? (size_t)sz : 0;
    fclose(f);
    return buf;
}

int main(int argc, char **argv) {
    if (argc < 4 || (argc - 2) % 2) {
        fprintf(stderr, "usage: %s slack_mult model.mars input.bin [...]\n", argv[0]);
        return 2;
    }
    const size_t slack = (size_t)strtoull(argv[1], NULL, 0);
    for (int i = 2; i + 1 < argc; i += 2) {
        size_t nm = 0, ni = 0;
        void *m = slurp(argv[i], &nm), *x = slurp(argv[i + 1], &ni);
        int err = 0;
        orc_graph_t *g = m && nm ? orc_graph_open(m, nm, slack, 1 << 16, &err) : NULL;
        if (!g || !x || orc_graph_set_input(g, 0, x, ni) != 0) {
            fprintf(stderr, "%s: cannot open (%d)\n", argv[i], err);
            return 1;
        }
        printf("rc %d\n", orc_graph_run(g));
        orc_graph_close(g);
        free(m);
        free(x);
    }
    return 0;
}
