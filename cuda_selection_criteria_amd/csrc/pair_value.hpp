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
// smhc_threshold is the ONE statement of criterion smh_c's per-pair count threshold for a minimum containment gamma
// (selhip_ctx_set_min_containment): with c / m the SuperMinHash estimate of J, I = J (a + b) / (1 + J) and
// C^ = I / a = c (a + b) / ((m + c) a), so C^ >= gamma iff c >= gamma m a / (a + b - gamma a).  The count kernels, pairs_count_kernel and
// selhip_smhc_threshold (the same function on the host) call it, nothing else spells the expression.
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

// the smallest count c in [0, m + 1] of equal buckets with C^ >= gamma for a pair of truncated cardinalities e_lo <= e_hi (m + 1: no
// count reaches it).  Every operation is rounded on its own, in the order written.
SELHIP_HD int smhc_threshold(int m, double gamma, unsigned long long e_lo, unsigned long long e_hi) {
    const double a = (double)e_lo, b = (double)e_hi;
    if (a == 0.0) return m + 1;                      // stage 2 never selects d = 0 under max containment; two empty rows do not survive
    const double num = (gamma * (double)m) * a;
    const double ga = gamma * a;
    const double den = (a + b) - ga;
    if (!(den > 0.0)) return m + 1;                  // gamma >= 1 + b / a: no count reaches it
    const double q = num / den;
    return q <= 0.0 ? 0 : q > (double)m ? m + 1 : (int)ceil(q);
}

// smh_value is the ONE statement of what a pair's value is under the SuperMinHash estimator (selhip_ctx_set_estimator, DESIGN.md
// section 18): a function of the count c of equal buckets, m and the pair's truncated cardinalities alone -- no HLL register is read.
//   SELHIP_MEASURE_JACCARD          c / m
//   SELHIP_MEASURE_MAX_CONTAINMENT  c (a + b) / ((m + c) a), a = min(e1, e2), b = max(e1, e2): the estimate C^ that smhc_threshold inverts
// Every operation is rounded on its own, in the order written.  No clamp (C^ may exceed 1); a = 0 is NaN explicitly, as in pair_value,
// and so is any other measure.  The emit forms of the count kernels and selhip_smh_value (the same function on the host) call it.
SELHIP_HD double smh_value(int measure, int m, int c, unsigned long long e1, unsigned long long e2) {
    if (measure == SELHIP_MEASURE_JACCARD) return (double)c / (double)m;
    const unsigned long long e_lo = e1 < e2 ? e1 : e2, e_hi = e1 < e2 ? e2 : e1;
    if (measure != SELHIP_MEASURE_MAX_CONTAINMENT || e_lo == 0) return bits2d(0x7FF8000000000000ull);
    const double a = (double)e_lo, b = (double)e_hi;
    const double num = (double)c * (a + b);
    const double den = ((double)m + (double)c) * a;
    return num / den;
}

}  // namespace selhip
