// pair_value.hpp -- the ONE statement of what a pair's value is under every HLL measure but the union size: stage 2 of the passes
// (ertl_select_kernel, dense_select_kernel) and matrix_kernel call it, nothing else spells these expressions.
// Part of the kernel translation unit selection_kernels.hip (included there behind include/selection_hip.h and ertl_mle.hpp), which is
// compiled with -ffp-contract=off: every operation below is one IEEE-754 double operation, in the order written.
//   e1, e2 = the pair's truncated cardinalities as doubles ((double)ecard), U = the Ertl-MLE estimate of the union's size
//   I = e1 + e2 - U                 the inclusion-exclusion estimate of |A n B|: the numerator of selection.cpp:287, left to right
//   SELHIP_MEASURE_JACCARD          I / U                       (selection.cpp:287 itself: the bits every pass has always produced)
//   SELHIP_MEASURE_INTERSECTION     I
//   SELHIP_MEASURE_CONTAINMENT      I / e1                      the share of the FIRST genome found in the second; not symmetric
//   SELHIP_MEASURE_MAX_CONTAINMENT  I / (e1 < e2 ? e1 : e2)     the share of the smaller genome found in the larger; symmetric
// No clamp and no abs, as for J: estimator noise may give a value below 0 or above 1.  A containment whose denominator is 0 (an empty
// sketch) is NaN -- never +-inf -- so `value >= tau` is false for it under every tau: such a pair is never selected.
// (e2 + e1 - U has the bits of e1 + e2 - U -- IEEE addition commutes -- so the value of (b, a) may be computed from the operands of (a, b).)
#pragma once

namespace selhip {

SELHIP_HD double pair_value(int measure, double e1, double e2, double U) {
    const double I = e1 + e2 - U;
    if (measure == SELHIP_MEASURE_JACCARD) return I / U;
    if (measure == SELHIP_MEASURE_INTERSECTION) return I;
    const double d = measure == SELHIP_MEASURE_CONTAINMENT ? e1 : (e1 < e2 ? e1 : e2);
    return d != 0.0 ? I / d : bits2d(0x7FF8000000000000ull);
}

}  // namespace selhip
