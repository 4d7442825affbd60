// rollout_tile.hpp — the policy-forward + sampling tile code shared by every rollout kernel of the MLP policy
// (frameworks/cleanrl.py:60-66 Policy.forward with action=None = models.py:41-62 + cleanrl.py:25-47): the standalone
// forward (rollout.hip), the fused Squared rollout (rollout.hip) and the env skeleton of the other families (rollout_env.hpp) run
// exactly this code, so the protocol path and every fused rollout give bit-identical numbers.
#pragma once
#include <type_traits>

#include "common.hpp"
#include "lane_ops.hpp"
#include "mlp_tile.hpp"
#include "philox.hpp"
#include "sampler.hpp"

namespace pfa {

// ---------------------------------------------------------------------------------------------
// Shared by the standalone forward and the fused rollout: a 256-thread workgroup (4 wavefronts) owns one
// 16-row tile.  Wave w computes hidden tiles m in {2w, 2w+1} and its K-slice of the heads; after a barrier
// thread (le, lo) = (tid/16, tid%16) owns output `lo` of row `le`.  Both kernels run exactly this code, so
// policy(obs) through the protocol and the fused rollout give bit-identical numbers.
// ---------------------------------------------------------------------------------------------
constexpr int kRollThreads = 256;
constexpr int kRollWaves = 4;
constexpr int kMW = kMT / kRollWaves;  // hidden tiles per wave

// Where a Default policy's tensors live (models.py:24-39), so that the same tile code serves the kernel-layout buffer of the 128-wide
// policy (W1 rows padded to the observation stride) and a module's own tensors in torch's shapes (any width; general.py).
struct MlpView {
    const float *w1;   // encoder.weight [hidden][ldw1], columns >= cols read as 0
    int ldw1, cols;
    const float *b1;   // encoder.bias [hidden]
    const float *w2;   // decoder.weight [a][hidden]
    const float *b2;   // decoder.bias [a]
    const float *wv;   // value_head.weight [hidden]
    const float *bv;   // value_head.bias [1]
    int a, hidden;
    __device__ __forceinline__ float w2v(int o, int u) const { return o < a ? w2[o * hidden + u] : (o == a ? wv[u] : 0.0f); }
    __device__ __forceinline__ float b2v(int o) const { return o < a ? b2[o] : (o == a ? bv[0] : 0.0f); }
};
inline MlpView mlp_view_of_flat(const float *params, int dp, int a) {   // the flat layout of include/pufferlib_amd.h (hidden 128)
    const MlpOffsets off = mlp_offsets(dp, a);
    return MlpView{params + off.w1, dp, dp, params + off.b1, params + off.w2, params + off.b2, params + off.wv, params + off.bv, a, kHidden};
}

// KS = k-steps (4 observation columns each) the forward issues.  Default: the whole padded row.  A launch whose true feature
// count fits fewer steps passes the smaller number: the dropped products are pad weight x pad observation = +0 added to the
// accumulator (like the gradient kernel's KKU, ppo_update.hip), and every rollout-mode kernel of a policy takes the same KS,
// so the protocol path and the fused path stay bit-identical.
// MW = hidden tiles (16 units each) per wave: hidden = 64 MW, i.e. 64 / 128 / 256 / 512 for MW = 1 / 2 / 4 / 8.  The W1 fragments
// of any of them fit the registers of a one-wave-per-SIMD workgroup (MW x KS <= 128 floats at a 64-float row).
template <int DP, int KS = DP / 4, int MW = kMW>
struct SliceFrags {
    float w1f[MW][KS], b1f[MW][4], w2f[MW][4], bo[4];
    __device__ __forceinline__ void load(const float *params, int a) {
        const MlpOffsets off = mlp_offsets(DP, a);
        const int wv = wave_id(), c = lane_id() & 15, g = lane_id() >> 4;
#pragma unroll
        for (int i = 0; i < MW; ++i) {
            const int m = MW * wv + i;
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) w1f[i][kk] = params[off.w1 + (16 * m + c) * DP + 4 * kk + g];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                b1f[i][r] = params[off.b1 + 16 * m + 4 * g + r];
                w2f[i][r] = w2v_at(params, off, a, c, 16 * m + 4 * g + r);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) bo[r] = wv == 0 ? b2v_at(params, off, a, 4 * g + r) : 0.0f;
    }
    __device__ __forceinline__ void load(const MlpView &p) {   // the same fragments from wherever the tensors live
        const int wv = wave_id(), c = lane_id() & 15, g = lane_id() >> 4;
#pragma unroll
        for (int i = 0; i < MW; ++i) {
            const int m = MW * wv + i;
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) w1f[i][kk] = 4 * kk + g < p.cols ? p.w1[(size_t)(16 * m + c) * p.ldw1 + 4 * kk + g] : 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                b1f[i][r] = p.b1[16 * m + 4 * g + r];
                w2f[i][r] = p.w2v(c, 16 * m + 4 * g + r);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) bo[r] = wv == 0 ? p.b2v(4 * g + r) : 0.0f;
    }
};

// Global rows -> padded LDS tile, all 256 threads.
template <int DP>
__device__ __forceinline__ void stage_rows(const float *src, long long first_row, long long rows, float *xs,
                                           int tile_rows = 16) {
    constexpr int XS = XTile<DP>::XS, V = DP / 4;
    for (int idx = threadIdx.x; idx < 16 * V; idx += kRollThreads) {
        const int r = idx / V, c4 = idx - r * V;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < tile_rows && first_row + r < rows) x = *reinterpret_cast<const float4 *>(src + (first_row + r) * DP + 4 * c4);
        float2 *d = reinterpret_cast<float2 *>(xs + r * XS + 4 * c4);
        d[0] = make_float2(x.x, x.y);
        d[1] = make_float2(x.z, x.w);
    }
}

// LDS tile -> global rows (dst row r at dst + (first_row + r) * row_stride floats), all 256 threads.
template <int DP>
__device__ __forceinline__ void unstage_rows(const float *xs, float *dst, long long first_row, long long rows, size_t row_stride,
                                             int tile_rows = 16) {
    constexpr int XS = XTile<DP>::XS, V = DP / 4;
    for (int idx = threadIdx.x; idx < tile_rows * V; idx += kRollThreads) {
        const int r = idx / V, c4 = idx - r * V;
        if (first_row + r < rows) {
            const float2 *sp = reinterpret_cast<const float2 *>(xs + r * XS + 4 * c4);
            const float2 lo2 = sp[0], hi2 = sp[1];
            *reinterpret_cast<float4 *>(dst + (size_t)(first_row + r) * row_stride + 4 * c4) = make_float4(lo2.x, lo2.y, hi2.x, hi2.y);
        }
    }
}

// unstage_rows in two halves, for a caller that wants other work between the LDS read and the global store (forward_slice's hook).
// FULL: the caller vouches that all 16 rows of the tile exist; tile_rows and the row guard are not looked at.  Where the tile is a
// whole number of passes of the workgroup (rows of 64 or 128 floats) the stores then stand in straight-line code, where the compiler
// can count them: a later wait for an older load becomes vmcnt(n) instead of a vmcnt(0) that also waits for these stores.
template <int DP, bool FULL>
struct RowStore {
    static constexpr int XS = XTile<DP>::XS, V = DP / 4, kPasses = (16 * V + kRollThreads - 1) / kRollThreads;
    const float *xs;
    float *dst;
    long long first_row, rows;
    size_t row_stride;
    int tile_rows;
    float2 lo2[kPasses], hi2[kPasses];
    __device__ __forceinline__ bool live(int j) const {
        if constexpr (FULL) {
            if (16 * V >= (j + 1) * kRollThreads) return true;
        }
        const int idx = threadIdx.x + j * kRollThreads;
        return idx < (FULL ? 16 : tile_rows) * V && (FULL || first_row + idx / V < rows);
    }
    __device__ __forceinline__ void read() {
#pragma unroll
        for (int j = 0; j < kPasses; ++j) {
            const int idx = threadIdx.x + j * kRollThreads, r = idx / V, c4 = idx - r * V;
            if (live(j)) {
                const float2 *sp = reinterpret_cast<const float2 *>(xs + r * XS + 4 * c4);
                lo2[j] = sp[0], hi2[j] = sp[1];
            }
        }
    }
    __device__ __forceinline__ void store() const {
#pragma unroll
        for (int j = 0; j < kPasses; ++j) {
            const int idx = threadIdx.x + j * kRollThreads, r = idx / V, c4 = idx - r * V;
            if (live(j))
                *reinterpret_cast<float4 *>(dst + (size_t)(first_row + r) * row_stride + 4 * c4) =
                    make_float4(lo2[j].x, lo2[j].y, hi2[j].x, hi2[j].y);
        }
    }
};
struct NoHook {
    __device__ __forceinline__ void read() {}
    __device__ __forceinline__ void store() const {}
};

// This wave's slice of models.Default.forward (models.py:41-62) for the 16 rows in xs -> part[wave][o * kPartStride + row].
// `hook` (a RowStore) rides along: its LDS read is issued behind the B operand reads and its global store behind the first layer's
// products.  The fused rollout stores its observation rows this way; in front of the forward, the store's read and the wait for it
// stood before the operand reads, two LDS latencies in sequence ahead of the first product.
template <int DP, int KS = DP / 4, int MW = kMW, class Hook = NoHook>   // MW = 1 or even
__device__ __forceinline__ void forward_slice(const SliceFrags<DP, KS, MW> &w, const float *xs, float (*part)[kPartFloats],
                                              Hook hook = Hook{}) {
    constexpr int XS = XTile<DP>::XS;
    const int wv = wave_id(), c = lane_id() & 15, g = lane_id() >> 4;
    f32x4 h[MW];
#pragma unroll
    for (int i = 0; i < MW; ++i) h[i] = f32x4{w.b1f[i][0], w.b1f[i][1], w.b1f[i][2], w.b1f[i][3]};
    // every B value of the row first, the products behind them: left to itself the compiler sinks each ds_read next to its products
    // and drains lgkmcnt in front of every group (ISA of round 4: seven exposed LDS latencies per step of the rollout's dependent
    // chain); same products in the same order, so the numbers do not change
    float bv[KS];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) bv[kk] = xs[c * XS + 4 * kk + g];
    __builtin_amdgcn_sched_barrier(0);
    hook.read();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
#pragma unroll
        for (int i = 0; i < MW; ++i) h[i] = mfma16(w.w1f[i][kk], bv[kk], h[i]);
    }
    hook.store();
    // the heads' contraction over this wave's 16 MW hidden units: two accumulator chains (even / odd tiles)
    // ReLU as max(bits, 0) on the integer view: one instruction where fmaxf is two (canonicalise + max), and exact — negative floats
    // and -0 are negative integers, positive floats pass unchanged (the gradient kernel's form, ppo_update.hip).  Only a NaN without
    // the sign bit differs: it stays a NaN where fmaxf(NaN, 0) is 0.
    const auto relu = [](float x) { return __int_as_float(max(__float_as_int(x), 0)); };
    f32x4 o0 = f32x4{w.bo[0], w.bo[1], w.bo[2], w.bo[3]}, o1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < MW; i += 2) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            o0 = mfma16(w.w2f[i][r], relu(h[i][r]), o0);
            if constexpr (MW >= 2) o1 = mfma16(w.w2f[i + 1][r], relu(h[i + 1][r]), o1);
        }
    }
    const f32x4 po = o0 + o1;  // partial out^T[o = 4g + r][row = c]
#pragma unroll
    for (int r = 0; r < 4; ++r) part[wv][(4 * g + r) * kPartStride + c] = po[r];
}

// Sum of the four waves' head partials for (row le, output lo), then sample_row16 (sampler.hpp).
__device__ __forceinline__ LaneSample sample_lanes(const float (*part)[kPartFloats], int le, int lo, int a, float q) {
    const int i = lo * kPartStride + le;
    const float mine = (part[0][i] + part[1][i]) + (part[2][i] + part[3][i]);
    return sample_row16(mine, lo, a, q);
}
__device__ __forceinline__ LaneSample sample_lanes_heads(const float (*part)[kPartFloats], int le, int lo, int a, uint32_t heads, float q) {
    const int i = lo * kPartStride + le;
    const float mine = (part[0][i] + part[1][i]) + (part[2][i] + part[3][i]);
    return sample_row16_heads(mine, lo, a, heads, q);
}

// Host side: the one map from a policy's row shape to the instantiation every rollout-mode kernel of that policy takes.
// DP = observation row stride, KS = forward k-steps: the 7x7 grid's 49 columns need 13 of the 64-float row's 16 (SliceFrags),
// MW = hidden tiles per wave (hidden = 64 MW).  `launch` is called with the Tile of the shape.
template <int DP_, int KS_, int MW_>
struct Tile {
    static constexpr int DP = DP_, KS = KS_, MW = MW_;
};
template <int MW, class Launch>
static void dispatch_stride(int obs_stride, int obs_dim, Launch launch) {
    if (obs_stride == 64 && obs_dim > 48 && obs_dim <= 52) return launch(Tile<64, 13, MW>{});
    switch (obs_stride) {
        case 16: return launch(Tile<16, 4, MW>{});
        case 32: return launch(Tile<32, 8, MW>{});
        case 64: return launch(Tile<64, 16, MW>{});
    }
    if constexpr (MW == kMW) {   // rows of 96 / 128 floats: the 128-wide form only
        if (obs_stride == 96) return launch(Tile<96, 24, MW>{});
        return launch(Tile<128, 32, MW>{});
    }
}

// A Default policy as the tile kernels take it, from either descriptor form: the flat parameter buffer of the 128-wide family with
// its pfa_mlp_dims, or a pfa_mlp_view of a module's own tensors (hidden 64 / 128 / 256 / 512).  One checker per form; the standalone
// forward, the Squared rollout (rollout.hip) and the view form of the env skeleton (rollout_env.hpp) all launch through dispatch_tile.
struct TilePolicy {
    MlpView pv;
    int obs_dim, obs_stride;
    uint32_t heads;
};

inline int check_shape(bool flat, int hidden, int obs_dim, int obs_stride, int a, uint32_t heads) {
    if (flat) {
        PFA_REQUIRE(hidden == kHidden, "mlp: hidden must be %d (got %d)", kHidden, hidden);
    } else {
        PFA_REQUIRE(hidden == 64 || hidden == 128 || hidden == 256 || hidden == 512, "mlp view: hidden %d is not one of 64/128/256/512", hidden);
    }
    PFA_REQUIRE(valid_row_stride(obs_stride, flat ? 128 : 64),
                "mlp: obs_stride must be one of %s (got %d)", flat ? "16/32/64/96/128" : "16/32/64", obs_stride);
    PFA_REQUIRE(obs_dim >= 1 && obs_dim <= obs_stride, "mlp: obs_dim %d out of range", obs_dim);
    PFA_REQUIRE(a >= 1 && a <= 15, "mlp: num_actions must be in 1..15 (got %d)", a);
    PFA_REQUIRE(heads == 0 || (flat && heads_count(heads, a) >= 1), "mlp: head sizes 0x%x do not sum to num_actions %d", heads, a);
    return 0;
}
inline int check_dims(const pfa_mlp_dims *d) {
    PFA_REQUIRE(d != nullptr, "mlp: null dims");
    return check_shape(true, d->hidden, d->obs_dim, d->obs_stride, d->num_actions, d->heads);
}
inline int check_view(const pfa_mlp_view *p) {
    PFA_REQUIRE(p != nullptr, "mlp view: null");
    PFA_REQUIRE(p->w1 && p->b1 && p->w2 && p->b2 && p->wv && p->bv, "mlp view: null tensor");
    PFA_REQUIRE(p->ldw1 >= p->obs_dim, "mlp view: obs_dim %d / ldw1 %d out of range", p->obs_dim, p->ldw1);
    return check_shape(false, p->hidden, p->obs_dim, p->obs_stride, p->num_actions, 0);
}
inline int policy_of_flat(const float *params, const pfa_mlp_dims *d, TilePolicy *out) {
    if (int rc = check_dims(d)) return rc;
    PFA_REQUIRE(params, "mlp: null parameter buffer");
    *out = TilePolicy{mlp_view_of_flat(params, d->obs_stride, d->num_actions), d->obs_dim, d->obs_stride, d->heads};
    return 0;
}
inline int policy_of_view(const pfa_mlp_view *p, TilePolicy *out) {
    if (int rc = check_view(p)) return rc;
    *out = TilePolicy{MlpView{p->w1, p->ldw1, p->obs_dim, p->b1, p->w2, p->b2, p->wv, p->bv, p->num_actions, p->hidden}, p->obs_dim,
                      p->obs_stride, 0};
    return 0;
}

// hidden -> MW, then dispatch_stride: `launch` is called with the Tile of the policy's shape.  kOnlyDP != 0: the one row width the
// caller's env has (only the four widths of that row are instantiated); it equals what dispatch_stride gives that row.
template <int kOnlyDP = 0, class Launch>
static void dispatch_tile(const TilePolicy &p, Launch launch) {
    auto with_mw = [&](auto mw) {
        constexpr int MW = decltype(mw)::value;
        if constexpr (kOnlyDP != 0) {
            static_assert(kOnlyDP == 16 || kOnlyDP == 32, "a row dispatch_stride never trims");
            launch(Tile<kOnlyDP, kOnlyDP / 4, MW>{});
        } else {
            dispatch_stride<MW>(p.obs_stride, p.obs_dim, launch);
        }
    };
    switch (p.pv.hidden) {
        case 64: return with_mw(std::integral_constant<int, 1>{});
        case 128: return with_mw(std::integral_constant<int, 2>{});
        case 256: return with_mw(std::integral_constant<int, 4>{});
        default: return with_mw(std::integral_constant<int, 8>{});
    }
}

}  // namespace pfa
