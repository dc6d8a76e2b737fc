/* The launch-group rule of the planner and the run loop (op_form / op_span / op_head / op_is_mate, csrc/host/mars_internal.h) on hand-made op
 * arrays.  A stand-alone host program: no device layer is linked, every array is allocated at exactly its length so that a read past the end
 * shows under AddressSanitizer (tests/test_plan_groups_cpu.py builds and runs it). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mars_internal.h"

static mars_model_ext_t M;
static int failures;

#define CHECK(cond) do { if (!(cond)) { printf("plan_groups: line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

/* a plan of n plain int8 convolutions, in a block of exactly n ops */
static mars_op_t *plan(int n) {
    free(M.ops);
    M.ops = (mars_op_t *)calloc((size_t)n, sizeof(mars_op_t));
    M.n_ops = n;
    if (!M.ops) exit(2);
    for (int i = 0; i < n; i++) M.ops[i].kind = OP_CONV_I8;
    return M.ops;
}
/* the launch that starts at i: its form, its span, its members i .. i + span - 1 and nothing behind them */
static void expect(int i, int form, int span) {
    int g[4] = {-7, -7, -7, -7};
    CHECK(op_form(&M, i, g) == form);
    CHECK(op_span(&M, i) == span);
    CHECK(op_plain(&M, i) == (form == FORM_PLAIN)); /* (a flagged last op spans one op and is not plain) */
    for (int k = 0; k < 4; k++) CHECK(g[k] == (k < span ? i + k : -1));
}
static void expect_heads(const int *heads) {
    for (int i = 0; i < M.n_ops; i++) {
        CHECK(op_head(&M, i) == heads[i]);
        CHECK(op_is_mate(&M, i) == (heads[i] != i));
    }
}
/* the flags of form `form` on op i (side: the chained 1x1's, where the form has one) */
static void set_form(mars_op_t *o, int i, int form, int side) {
    switch (form) {
        case FORM_PAIR_F32: o[i].kind = OP_CONV_F32; /* (its mate's kind is not the rule's business: plan_check's) */ /* fall through */
        case FORM_PAIR: o[i].pair_next = 1; break;
        case FORM_BOTH_CHAIN: o[i].both_chain = side; /* fall through */
        case FORM_BOTH: o[i].pair_next = o[i].pair_both = 1; break;
        case FORM_POST: o[i].post_next = 1; break;
        case FORM_SPLIT_CHAIN: o[i].split_chain = side; /* fall through */
        case FORM_SPLIT: o[i].split_next = 1; break; /* (cv1's pair_next: set by the caller where the array holds cv1) */
        default: break;
    }
}

int main(void) {
    static const int forms[] = {FORM_PLAIN, FORM_PAIR, FORM_BOTH, FORM_BOTH_CHAIN, FORM_POST, FORM_SPLIT, FORM_SPLIT_CHAIN, FORM_PAIR_F32};
    static const int spans[] = {1, 2, 2, 3, 2, 3, 4, 2};
    CHECK(form_span(-1) == 0 && form_span(FORM_COUNT) == 0 && form_span(FORM_BAD) == 1);
    for (int f = 0; f < 8; f++) {
        const int form = forms[f], span = spans[f];
        CHECK(form_span(form) == span);
        for (int side = 1; side <= 2; side++) {
            /* the form in the middle of a plan: a plain op in front of it and one behind */
            mars_op_t *o = plan(span + 2);
            set_form(o, 1, form, side);
            if (span >= 3 && form != FORM_BOTH_CHAIN) o[2].pair_next = 1; /* cv1 of a split group keeps its flag */
            expect(0, FORM_PLAIN, 1);
            expect(1, form, span);
            expect(1 + span, FORM_PLAIN, 1);
            int heads[6] = {0, 1, 1, 1, 1, 1};
            heads[1 + span] = 1 + span;
            expect_heads(heads);
            /* ... at the very end of the plan */
            o = plan(span);
            set_form(o, 0, form, side);
            if (span >= 3 && form != FORM_BOTH_CHAIN) o[1].pair_next = 1;
            expect(0, form, span);
            for (int i = 0; i < span; i++) CHECK(op_head(&M, i) == 0);
            /* ... cut short by the end of the plan, by 1 .. span - 1 ops: an error that owns the ops left, and no member beyond them */
            for (int n = 1; n < span; n++) {
                o = plan(n);
                set_form(o, 0, form, side);
                expect(0, FORM_BAD, n);
                for (int i = 0; i < n; i++) CHECK(op_head(&M, i) == 0);
            }
        }
    }
    { /* cv1 and cv2 of a split group are mates of the split: cv1's own pair_next starts no pair, although op_form AT cv1 reads as one */
        mars_op_t *o = plan(4);
        o[0].split_next = 1; o[1].pair_next = 1;
        expect(0, FORM_SPLIT, 3);
        expect(1, FORM_PAIR, 2);
        const int heads[] = {0, 0, 0, 3};
        expect_heads(heads);
    }
    { /* two groups back to back: a pair right behind a split + chain group is a head, and so is the post launch behind that pair */
        mars_op_t *o = plan(9);
        o[0].split_next = 1; o[0].split_chain = 2; o[1].pair_next = 1;
        o[4].pair_next = 1;
        o[6].post_next = 1;
        expect(0, FORM_SPLIT_CHAIN, 4);
        expect(4, FORM_PAIR, 2);
        expect(6, FORM_POST, 2);
        const int heads[] = {0, 0, 0, 0, 4, 4, 6, 6, 8};
        expect_heads(heads);
    }
    for (int side = 1; side <= 2; side++) { /* D behind a one-tile pair, reading either side; a second such group right behind it */
        mars_op_t *o = plan(6);
        o[0].pair_next = o[0].pair_both = 1; o[0].both_chain = side; o[0].both_elide = side == 1;
        o[3].pair_next = o[3].pair_both = 1; o[3].both_chain = 3 - side;
        expect(0, FORM_BOTH_CHAIN, 3);
        expect(3, FORM_BOTH_CHAIN, 3);
        const int heads[] = {0, 0, 0, 3, 3, 3};
        expect_heads(heads);
    }
    { /* a one-tile pair's flags without pair_next name no group (plan_check rejects the plan); both_chain without pair_both is a plain pair */
        mars_op_t *o = plan(3);
        o[0].pair_both = 1; o[0].both_chain = 1;
        expect(0, FORM_PLAIN, 1);
        o[0].pair_both = 0; o[0].pair_next = 1;
        expect(0, FORM_PAIR, 2);
    }
    { /* the float pair, between an int8 pair and a plain float convolution */
        mars_op_t *o = plan(5);
        o[0].pair_next = 1;
        o[2].kind = o[3].kind = o[4].kind = OP_CONV_F32;
        o[2].pair_next = 1;
        expect(0, FORM_PAIR, 2);
        expect(2, FORM_PAIR_F32, 2);
        expect(4, FORM_PLAIN, 1);
        const int heads[] = {0, 0, 2, 2, 4};
        expect_heads(heads);
    }
    free(M.ops);
    if (failures) return 1;
    printf("plan_groups: ok\n");
    return 0;
}
