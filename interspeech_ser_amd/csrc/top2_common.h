// (top-1 value, its index, top-2 value) of a set, and the merge of two such triples: what ser_dec_select_v (decode.hip) and ser_ctc_greedy_v
// (ctc.hip) reduce a row of logits with.  The caller maps NaN to +inf on the way in, so plain comparisons order everything.  The triple of
// a union is a function of the multiset alone -- max, the lowest index of the max and the second value (the max again when it occurs
// twice) -- so the merge is associative and commutative and no split of a row over lanes changes a bit of the result.
#pragma once
#include "ser_common.h"

struct Top2 { float v1; int i1; float v2; };
__device__ __forceinline__ Top2 top2_merge(Top2 x, Top2 y) {
    const bool xw = x.v1 > y.v1 || (x.v1 == y.v1 && x.i1 < y.i1);             // the lowest index wins a tie (torch.argmax)
    Top2 r;
    r.v1 = xw ? x.v1 : y.v1;
    r.i1 = xw ? x.i1 : y.i1;
    r.v2 = xw ? fmaxf(x.v2, y.v1) : fmaxf(y.v2, x.v1);
    return r;
}
