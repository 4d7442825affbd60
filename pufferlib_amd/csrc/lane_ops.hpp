// lane_ops.hpp — reductions over the 16 lanes of a DPP row with data-parallel-primitive moves (one VALU op each)
// instead of ds_bpermute round trips through the LDS pipe: quad_perm[1,0,3,2], quad_perm[2,3,0,1], row_half_mirror,
// row_mirror.  After the four steps every lane of the row holds the reduction of all 16.
#pragma once
#include "common.hpp"

namespace pfa {

template <int CTRL>
__device__ __forceinline__ float dpp_f(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false));
}

constexpr int kDppXor1 = 0xB1;         // quad_perm [1,0,3,2]
constexpr int kDppXor2 = 0x4E;         // quad_perm [2,3,0,1]
constexpr int kDppHalfMirror = 0x141;  // lane i <-> 7-i within each 8
constexpr int kDppMirror = 0x140;      // lane i <-> 15-i within the row

// The same moves with bound_ctrl set.  Every lane of these four controls has a valid source, so the value is the same; what changes
// is that the compiler may fold the move into ANY consumer (v_max_i32_dpp, v_min_i32_dpp), not only into one for which the `old`
// operand 0 is the identity (v_add_f32_dpp).
template <int CTRL>
__device__ __forceinline__ int dpp_bc(int x) {
    return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xf, 0xf, true);
}
__device__ __forceinline__ int row16_max_i32(int x) {   // one v_max_i32_dpp per step
    x = max(x, dpp_bc<kDppXor1>(x));
    x = max(x, dpp_bc<kDppXor2>(x));
    x = max(x, dpp_bc<kDppHalfMirror>(x));
    x = max(x, dpp_bc<kDppMirror>(x));
    return x;
}
__device__ __forceinline__ int row16_min_i32(int x) {   // one v_min_i32_dpp per step
    x = min(x, dpp_bc<kDppXor1>(x));
    x = min(x, dpp_bc<kDppXor2>(x));
    x = min(x, dpp_bc<kDppHalfMirror>(x));
    x = min(x, dpp_bc<kDppMirror>(x));
    return x;
}

// Bits of a float as an integer that orders like the float (negative floats have their magnitude bits flipped); its own inverse.
__device__ __forceinline__ int float_order_key(int bits) { return bits ^ ((bits >> 31) & 0x7fffffff); }

// Row maximum of non-NaN floats (-inf included), as an integer maximum of the order keys.  fmaxf on a DPP move is five instructions
// per step: the compiler cannot see that the moved value is canonical, so a `v_max x, x` stands between the move and the maximum
// and the move cannot be folded.  The integer form is 3 + 4 + 3 instructions and returns the same number; of +0 and -0 it returns +0
// (the callers use the maximum only as x - mx under exp and as mx + log(sum >= 1), where the sign of a zero is lost).  A NaN input
// gives a NaN or an arbitrary maximum instead of being skipped: every caller's row is NaN throughout in that case (exp(x - mx) of
// the NaN lane poisons the sum).
__device__ __forceinline__ float row16_max(float x) {
    return __int_as_float(float_order_key(row16_max_i32(float_order_key(__float_as_int(x)))));
}

// Fixed combination order -> the same bits on every lane and in every kernel that uses it.
__device__ __forceinline__ float row16_sum(float x) {
    x = x + dpp_f<kDppXor1>(x);
    x = x + dpp_f<kDppXor2>(x);
    x = x + dpp_f<kDppHalfMirror>(x);
    x = x + dpp_f<kDppMirror>(x);
    return x;
}

// argmax with the lowest index winning ties (torch.argmax's rule on CPU): the lexicographic maximum of (value, -index), taken as
// the row maximum of the value and then the row minimum of `value == maximum ? idx : 16`.
// `best` must be >= +0 or -inf on every lane (the sampler's p / q, -inf on lanes outside the head): on that domain the bit pattern
// compared as a signed integer orders like the float and equal values have equal bits, so no float compare (and no canonicalising
// instruction) is needed.  `idx` is the lane's own column, 0..15.  A -inf lane wins only if the whole row is -inf.
__device__ __forceinline__ void row16_argmax(float &best, int &idx) {
    const int bits = __float_as_int(best);
    const int top = row16_max_i32(bits);
    idx = row16_min_i32(bits == top ? idx : 16);
    best = __int_as_float(top);
}

}  // namespace pfa
