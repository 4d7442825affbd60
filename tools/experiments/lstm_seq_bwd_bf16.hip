// lstm_seq_bwd_bf16.hip — EXPERIMENT (not product code, not in the build): lstm_seq_bwd_kernel in the bf16x6 product form, the
// counterpart of csrc/lstm_seq_bf16.hip's forward.  Bit-for-bit deterministic and within the float64 bound of
// tests/test_gpu_lstm_seq_bf16.py on all six cases when it was wired in (pfa_lstm_seq_path bit 1), but SLOWER than the fp32 kernel on
// the c3 bench shape (8192 rows x 16 steps, three alternating runs each): 350.6 us per launch against 323.8 (spread 0.3), so the fp32
// kernel stays under the switch (profiles/r07_lstm_seq_bf16_ab.json, lab notebook "The recurrent kernels in the bf16x6 form").
// 256 VGPRs + 254 AGPRs (FULL) / 222 (guarded), 0 spilled, 0 bytes of scratch, 99 840 bytes of LDS.
//
// Design: the cell backward writes the fp32 dG to HBM as before and its three bf16 planes (32 rows x 512, row stride 1040 bytes) to LDS;
// [dxe | dh_{t-1}]^T = Wcat^T dG^T runs over the 512 gate columns in 16 slabs of 32, two weight groups per slab (bf_stream_product<16, 4>
// of csrc/lstm_seq_bf16.hpp); the gate-bias column sums are taken from the fp32 values in registers (gsum, one 16-lane row sum at the
// end).  Suspects for the lost time, none measured: the split of 64 dG values per lane and step (~ 400 VALU + 48 ds_write_b64 on the
// step's serial part, in front of the barrier), and a weight stream of 768 KB per workgroup and step against a shorter product.
//
// To try it again: paste the pack branch into lstm_pack_split_kernel (a second destination), the kernel and launcher into
// csrc/lstm_seq_bf16.hip, set bit 1 of kSeqBfShip and dispatch on it in pfa_lstm_seq_backward.
#include "lane_ops.hpp"
#include "lstm_seq_bf16.hpp"

namespace pfa {

// the backward operand of the pack kernel: tile = 4 s + kt of wave w,  Wcat[32 s + 8 g + e][k(w, kt, c)], k as in lstm_pack_bwd_kernel
//     const int s = tile >> 2, kt = tile & 3;
//     const int k = 32 * w + 16 * (kt & 1) + c;
//     const float *src = params + ((kt >> 1) ? lo.w_hh : lo.w_ih) + k;
//     for (int e = 0; e < 8; ++e) x[e] = src[(32 * s + 8 * g + e) * kLH];

// ------------------------------------------------------------------------------------------------------------------------ backward
template <bool FULL>
__global__ void __launch_bounds__(kLstmThreads, 1) lstm_seq_bwd_bf16_kernel(const float *__restrict__ gates_act, const float *__restrict__ Cs,
                                                                          const float *__restrict__ xe, const float *__restrict__ dh_heads,
                                                                          long long R, int Th, const unsigned char *__restrict__ wsplit_bwd,
                                                                          float *__restrict__ dG, float *__restrict__ dxe,
                                                                          float *__restrict__ bias_partial) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // [3 pieces][32 rows][kGRowB]: the dG tile
    const int lane = lane_id(), wv = wave_id(), c = lane & 15, g = lane >> 4;
    const float4 *wp = reinterpret_cast<const float4 *>(wsplit_bwd + (size_t)__builtin_amdgcn_readfirstlane(wv) * (kSeqBfTiles * 3 * 1024));
    const long long first = (long long)blockIdx.x * kSeqRows;
    const int uoff = 32 * wv + 4 * g;  // this lane's units: uoff + 16 sub + r

    f32x4 dc[kSeqRT][2], dhrec[kSeqRT][2], xsum[2], gsum[2][4];   // gsum[sub][gate]: this lane's part of the gate-bias column sums
#pragma unroll
    for (int rt = 0; rt < kSeqRT; ++rt)
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) dc[rt][sub] = dhrec[rt][sub] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
        xsum[sub] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q) gsum[sub][q] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    // inputs of one step's cell backward, fetched during the previous product, one load per weight group (lstm_seq_bwd_kernel's)
    constexpr int kIn = 12;
    float4 in[kSeqRT][kIn], xv[kSeqRT][2], ccur[kSeqRT][2];
    auto fetch = [&](int k, int tt) {
        const int rt = k / kIn, j = k % kIn;
        const long long row = first + 16 * rt + c;
        if (!FULL && row >= R) {
            in[rt][j] = make_float4(0.f, 0.f, 0.f, 0.f);
            return;
        }
        const size_t tr = (size_t)tt * R + row;
        if (j < 8)
            in[rt][j] = *reinterpret_cast<const float4 *>(gates_act + tr * kLG + 128 * (j >> 1) + 16 * (j & 1) + uoff);
        else if (j < 10)
            in[rt][j] = *reinterpret_cast<const float4 *>(Cs + tr * kLH + 16 * (j - 8) + uoff);  // c_{tt-1}
        else
            in[rt][j] = *reinterpret_cast<const float4 *>(dh_heads + tr * kLH + 16 * (j - 10) + uoff);
    };
    auto fetch_x = [&](int k, int tt) {
        const int rt = k >> 1, sub = k & 1;
        const long long row = first + 16 * rt + c;
        xv[rt][sub] = (FULL || row < R) ? *reinterpret_cast<const float4 *>(xe + ((size_t)tt * R + row) * kLH + 16 * sub + uoff) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
#pragma unroll
    for (int k = 0; k < kSeqRT * kIn; ++k) fetch(k, Th - 1);
#pragma unroll
    for (int rt = 0; rt < kSeqRT; ++rt)
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const long long row = first + 16 * rt + c;
            ccur[rt][sub] = (FULL || row < R) ? *reinterpret_cast<const float4 *>(Cs + ((size_t)Th * R + row) * kLH + 16 * sub + uoff) : make_float4(0.f, 0.f, 0.f, 0.f);
        }

    for (int t = Th - 1; t >= 0; --t) {
        BfFrag ring[kSeqBfRing][6];
        const Stream ws = stream_begin(wp);
        bf_ring_prefetch(ws, ring);  // ahead of this step's stores in the memory queue
        // ---- cell backward, elementwise on (row c, units uoff + 16 sub + r); rows past R hold zeros throughout ------------------
#pragma unroll
        for (int rt = 0; rt < kSeqRT; ++rt) {
            const long long row = first + 16 * rt + c;
            const bool ok = FULL || row < R;
            float4 *dgo = reinterpret_cast<float4 *>(dG + ((size_t)t * R + (ok ? row : 0)) * kLG + uoff);
            unsigned char *dgl = smem + (16 * rt + c) * kGRowB + uoff * 2;
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                const float4 vi = in[rt][0 + sub], vf = in[rt][2 + sub], vg = in[rt][4 + sub], vo = in[rt][6 + sub];
                const float4 vcp = in[rt][8 + sub], vcn = ccur[rt][sub], vdh = in[rt][10 + sub];
                const float ai[4] = {vi.x, vi.y, vi.z, vi.w}, af[4] = {vf.x, vf.y, vf.z, vf.w};
                const float ag[4] = {vg.x, vg.y, vg.z, vg.w}, ao[4] = {vo.x, vo.y, vo.z, vo.w};
                const float acp[4] = {vcp.x, vcp.y, vcp.z, vcp.w}, acn[4] = {vcn.x, vcn.y, vcn.z, vcn.w};
                const float adh[4] = {vdh.x, vdh.y, vdh.z, vdh.w};
                f32x4 gq4[4];   // d loss / d gate pre-activations i, f, g, o
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float tc = tanh_f(acn[r]);
                    const float dhx = adh[r] + dhrec[rt][sub][r];  // heads path + recurrent path
                    const float d_o = dhx * tc;
                    const float d_c = dhx * ao[r] * (1.0f - tc * tc) + dc[rt][sub][r];
                    gq4[0][r] = d_c * ag[r] * ai[r] * (1.0f - ai[r]);
                    gq4[1][r] = d_c * acp[r] * af[r] * (1.0f - af[r]);
                    gq4[2][r] = d_c * ai[r] * (1.0f - ag[r] * ag[r]);
                    gq4[3][r] = d_o * ao[r] * (1.0f - ao[r]);
                    dc[rt][sub][r] = d_c * af[r];
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    bf_put4(dgl + (128 * q + 16 * sub) * 2, kGPlaneB, gq4[q][0], gq4[q][1], gq4[q][2], gq4[q][3]);
                    if (ok) dgo[(128 * q + 16 * sub) / 4] = make_float4(gq4[q][0], gq4[q][1], gq4[q][2], gq4[q][3]);
                    gsum[sub][q] += gq4[q];
                }
                ccur[rt][sub] = vcp;  // c_{t-1} is the next iteration's c_t
            }
        }
        __syncthreads();
        // ---- [dxe | dh_{t-1}]^T = Wcat^T dG^T, with next step's inputs streaming in ---------------------------------
        f32x4 acc[kSeqRT][4];
#pragma unroll
        for (int rt = 0; rt < kSeqRT; ++rt)
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) acc[rt][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const bool more = t > 0;
        bf_stream_product<kLG / 32, 4, kGRowB, kGPlaneB>(ws, smem + c * kGRowB + 16 * g, ring, acc, [&](int gq) {
            if (gq < 4) fetch_x(gq, t);
            else if (more && gq - 4 < kSeqRT * kIn) fetch(gq - 4, t - 1);
        });
        // ---- outputs: dxe (with relu') to global, dh_{t-1} stays in registers ------------------------------------------
#pragma unroll
        for (int rt = 0; rt < kSeqRT; ++rt) {
            const long long row = first + 16 * rt + c;
            const bool ok = FULL || row < R;
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                dhrec[rt][sub] = acc[rt][2 + sub];
                const float4 x4 = xv[rt][sub];
                f32x4 d = acc[rt][sub];
                d[0] = x4.x > 0.0f ? d[0] : 0.0f;
                d[1] = x4.y > 0.0f ? d[1] : 0.0f;
                d[2] = x4.z > 0.0f ? d[2] : 0.0f;
                d[3] = x4.w > 0.0f ? d[3] : 0.0f;
                xsum[sub] += d;
                if (ok) *reinterpret_cast<float4 *>(dxe + ((size_t)t * R + row) * kLH + uoff + 16 * sub) = make_float4(d[0], d[1], d[2], d[3]);
            }
        }
        __syncthreads();  // every wave is done with the dG planes before the next step overwrites them
    }

    // ---- per-workgroup column sums (bias gradients): each of the 640 columns belongs to one (wave, g, sub, r), summed over its 16 row lanes
    float *bp = bias_partial + (size_t)blockIdx.x * kBiasCols;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float s = row16_sum(gsum[sub][q][r]);
                if (c == 0) bp[128 * q + 16 * sub + uoff + r] = s;
            }
            const float s = row16_sum(xsum[sub][r]);
            if (c == 0) bp[kLG + 16 * sub + uoff + r] = s;
        }
}


template <bool FULL>
static int seq_bwd_bf16_launch_full(unsigned grid, hipStream_t stream, const float *gates_act, const float *Cs, const float *xe,
                                    const float *dh_heads, long long R, int Th, const unsigned char *wsplit_bwd, float *dG, float *dxe,
                                    float *bias_partial) {
    static bool attr = false;
    if (!attr) {
        PFA_CHECK_HIP(hipFuncSetAttribute((const void *)lstm_seq_bwd_bf16_kernel<FULL>, hipFuncAttributeMaxDynamicSharedMemorySize, 3 * kGPlaneB));
        attr = true;
    }
    hipLaunchKernelGGL(lstm_seq_bwd_bf16_kernel<FULL>, dim3(grid), dim3(kLstmThreads), 3 * kGPlaneB, stream, gates_act, Cs, xe, dh_heads, R, Th,
                       wsplit_bwd, dG, dxe, bias_partial);
    return 0;
}

int lstm_seq_bwd_bf16_launch(hipStream_t stream, const float *gates_act, const float *Cs, const float *xe, const float *dh_heads, long long R,
                             int Th, const void *wsplit_bwd, float *dG, float *dxe, float *bias_partial) {
    PFA_REQUIRE((uintptr_t)wsplit_bwd % 16 == 0, "lstm_seq_backward: the split pack must be 16-byte aligned");
    const unsigned grid = (unsigned)((R + kSeqRows - 1) / kSeqRows);
    const unsigned char *wp = (const unsigned char *)wsplit_bwd;
    if (int rc = R % kSeqRows == 0 ? seq_bwd_bf16_launch_full<true>(grid, stream, gates_act, Cs, xe, dh_heads, R, Th, wp, dG, dxe, bias_partial)
                                   : seq_bwd_bf16_launch_full<false>(grid, stream, gates_act, Cs, xe, dh_heads, R, Th, wp, dG, dxe, bias_partial))
        return rc;
    PFA_LAUNCH_CHECK();
    return 0;
}


}  // namespace pfa
