// hll_fold.hpp -- the ONE statement of how a HyperLogLog sketch of precision p folds into the sketch of a lower precision p_aux that
// the same hashes would have built: hll_fold_kernel (kernel_fold.cuh) and selhost_hll_fold (host/selection_host.cpp) call it, nothing
// else spells these expressions.  Shared by host and device like ertl_mle.hpp (which defines SELHIP_HD) and pair_value.hpp.
//
// The reference's HLL (sketch/include/sketch/hll.h:886-888, restated in kernel_sketch.cuh:hll_slot and synth.hpp:synth_hll_slot) puts a
// hash h into register h >> (64 - p) with rank clz(((h << 1) | 1) << (p - 1)) + 1, and a register keeps the largest rank it saw.  With
// d = p - p_aux the index of precision p splits into the index g of precision p_aux (its top p_aux bits) and the d DROPPED bits t, which
// at precision p_aux are the first d bits the rank counts:
//   t != 0   the rank at p_aux is the position of t's leading one among those d bits: clz_d(t) + 1 = d - floor(log2 t), whatever
//            the register holds, as long as it is not empty
//   t == 0   all d dropped bits are zero and the count goes on where the rank at p stopped: d + r
// so    out[g] = max over t in [0, 2^d) with r = in[(g << d) | t], r != 0 of fold_contrib(r, t, d)        (0 if every r is 0).
// The largest legal r is 64 - p + 1 and folds to 64 - p_aux + 1, the cap of the direct sketch; registers above it cannot come from
// the builder and what they fold to is unspecified (nothing validates them).
//
// fold_contrib does not increase along t over the non-empty registers of a group (t == 0 gives more than d, t > 0 gives
// d - floor(log2 t) <= d), so the combine of a run of consecutive offsets is the contribution of the run's FIRST non-empty register:
// a caller that walks a run in ascending t may stop at it.
#pragma once

namespace selhip {

// what the non-empty register r at dropped bits t contributes to its output register (0 for an empty one); t < 2^d, d <= 16
SELHIP_HD unsigned fold_contrib(unsigned r, unsigned t, unsigned d) {
    if (r == 0) return 0;
    return t == 0 ? d + r : d - (31u - (unsigned)__builtin_clz(t));
}

// two contributions to one output register
SELHIP_HD unsigned fold_combine(unsigned a, unsigned b) { return a > b ? a : b; }

}  // namespace selhip
