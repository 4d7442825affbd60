// cnn_heads.hip — the head side of the NatureCNN policy (pufferlib/models.py:152-157 decode_actions: actor Linear(H, A),
// value_fn Linear(H, 1)) on the H-wide hidden vector the conv stack + Linear(flat_size, H) of csrc/igemm.hip produce (H = 512 or 128):
//   cnn_heads_sample   rollout: logits, value, sample_logits (cleanrl.py:25-47) -> action, log-prob, entropy, value
//   cnn_heads_loss     training: the same heads, the PPO loss of clean_pufferl.py:202-238, d loss / d (head outputs) [rows][16],
//                      d loss / d (pre-ReLU hidden) [rows][H], the six loss sums (f64, (hi, lo) float pairs); the loss itself is
//                      ppo_row_loss.hpp's, shared with the LSTM and width-general heads kernels
//   cnn_heads_eval     policy(frames, action=...): log-prob of GIVEN actions, entropy, value (the rollout's bits for the action it drew)
//   cnn_heads_eval_backward  its backward for arbitrary upstream gradients: d / d (head outputs) [rows][16], d / d (pre-ReLU hidden)
//   cnn_gather_frames  the uint8 frames of a chunk of minibatch rows, copied next to each other (rows of a minibatch are
//                      bptt_horizon-long segments of the env-major experience, clean_pufferl.py:455-457)
// 16 lanes per row (lane lo = head output lo), the row's hidden vector in LDS, head weights in LDS (padded rows: conflict-free),
// the 16-lane log-softmax / arg-max pieces shared with the MLP and LSTM policies (sampler.hpp), so all three sample and score
// with identical arithmetic.  The hidden width is a template argument (512: the Atari binding, 128: crafter / dm_lab / butterfly) or, for
// any other multiple of 16 up to 1024, a run-time argument of the same code (the LDS carve follows the width).  More than 15 actions: the row kernels of csrc/general.hip on head outputs computed by pfa_igemm_rows.  VALU work: 2 x H x (A + 1) flop per row against ~56 MFLOP in the conv stack.
#include <type_traits>

#include "common.hpp"
#include "lane_ops.hpp"
#include "mlp_tile.hpp"
#include "ppo_row_loss.hpp"
#include "ppo_tile.hpp"
#include "sampler.hpp"

namespace pfa {

constexpr int kCnnMaxH = 1024;    // LDS: 16 head rows of H + 1 floats and 16 hidden rows of H floats (129 KB at 1024, of 160 KB)

struct CnnHeads {   // actor.weight [A][H], actor.bias [A], value_fn.weight [1][H], value_fn.bias [1] (torch layout), H = the hidden width
    const float *w2, *b2, *wv, *bv;
    int a;
};

// HT: the hidden width as a template argument (512, 128), or 0 = the run-time width `hrt` (any multiple of 16)
template <int HT>
__device__ __forceinline__ void cnn_stage_heads(const CnnHeads &hd, float *w2v /* [16][H + 1] */, float *b2v, int hrt) {
    const int H = HT ? HT : hrt;
    for (int i = threadIdx.x; i < kOut * H; i += blockDim.x) {
        const int o = i / H, u = i - o * H;
        w2v[o * (H + 1) + u] = o < hd.a ? hd.w2[o * H + u] : (o == hd.a ? hd.wv[u] : 0.0f);
    }
    for (int i = threadIdx.x; i < kOut; i += blockDim.x) b2v[i] = i < hd.a ? hd.b2[i] : (i == hd.a ? hd.bv[0] : 0.0f);
}
template <int HT>
__device__ __forceinline__ float cnn_head_dot(const float *hrow, const float *w2v, const float *b2v, int lo, int hrt) {
    const int H = HT ? HT : hrt;
    float acc = b2v[lo];
    const float *w = w2v + lo * (H + 1);
#pragma unroll 8
    for (int u = 0; u < H; ++u) acc = fmaf(hrow[u], w[u], acc);   // k-ordered fma chain, like nn.Linear's fp32 dot
    return acc;
}

// The dynamic LDS of the four heads kernels (cnn_heads_lds(H) bytes): head weights [16][H + 1], their biases [16], hidden rows [16][H]
struct CnnLds {
    float *lds;
    int H;
    __device__ __forceinline__ float *w2v() const { return lds; }
    __device__ __forceinline__ float *b2v() const { return lds + kOut * (H + 1); }
    __device__ __forceinline__ float *hs() const { return b2v() + kOut; }
};
// hidden rows 16 tile .. 16 tile + 15 into hs (zeros past the end), between the barriers that fence the previous tile's readers and
// publish this one
template <int HT>
__device__ __forceinline__ void cnn_stage_rows(const float *h, float *hs, long long tile, long long rows, int hrt) {
    const int H = HT ? HT : hrt;
    __syncthreads();
    for (int i = threadIdx.x; i < 16 * H; i += 256) {
        const long long r = tile * 16 + i / H;
        hs[i] = r < rows ? h[r * H + i % H] : 0.0f;
    }
    __syncthreads();
}

template <int HT>
__global__ void __launch_bounds__(256) cnn_heads_sample_kernel(const float *h, int hrt, long long rows, CnnHeads hd, const float *noise, uint64_t seed,
                                                              uint64_t step, long long row_offset, long long *actions, float *logprob,
                                                              float *entropy, float *value) {
    extern __shared__ float lds[];
    const int H = HT ? HT : hrt;
    const CnnLds m{lds, H};
    float *w2v = m.w2v(), *b2v = m.b2v(), *hs = m.hs();
    cnn_stage_heads<HT>(hd, w2v, b2v, hrt);
    const int le = threadIdx.x >> 4, lo = threadIdx.x & 15, a = hd.a;
    const long long tiles = (rows + 15) / 16;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        cnn_stage_rows<HT>(h, hs, tile, rows, hrt);
        const long long row = tile * 16 + le;
        const bool ok = row < rows;
        const float mine = cnn_head_dot<HT>(hs + le * H, w2v, b2v, lo, hrt);
        const float q = ok ? noise_lane(noise ? noise + row * a : nullptr, seed, step, (uint64_t)(row_offset + row), lo, a) : 1.0f;
        const LaneSample sm = sample_row16(mine, lo, a, q);
        if (ok && lo == 0) {
            actions[row] = sm.action;
            logprob[row] = sm.logprob;
            if (entropy) entropy[row] = sm.entropy;
            value[row] = sm.value;
        }
    }
}

// d loss / d h[u] = sum_o d_o W2v[o][u] for the row of the 16 lanes that hold d (lane lo: d of head output lo); lane lo owns
// u = lo, lo + 16, ...  (the hidden vector is relu(Linear(...)): hand back d loss / d (pre-activation), i.e. masked by relu')
template <int HT>
__device__ __forceinline__ void cnn_heads_dh(float d, const float *w2v, const float *hs, int le, int lo, int a, bool ok, long long row, float *dh,
                                             int hrt) {
    const int H = HT ? HT : hrt;
    if (HT) {
        float dhv[(HT ? HT : 16) / 16];
#pragma unroll
        for (int j = 0; j < HT / 16; ++j) dhv[j] = 0.0f;
        for (int o = 0; o <= a; ++o) {
            const float d_o = __shfl(d, (lane_id() & 48) | o, 64);
#pragma unroll
            for (int j = 0; j < HT / 16; ++j) dhv[j] = fmaf(d_o, w2v[o * (HT + 1) + lo + 16 * j], dhv[j]);
        }
        if (ok) {
#pragma unroll
            for (int j = 0; j < HT / 16; ++j) dh[row * HT + lo + 16 * j] = hs[le * HT + lo + 16 * j] > 0.0f ? dhv[j] : 0.0f;
        }
    } else {   // any width: the same fma chains over o, eight columns of the lane at a time
        for (int j0 = 0; j0 < H / 16; j0 += 8) {
            float dhv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) dhv[j] = 0.0f;
            for (int o = 0; o <= a; ++o) {
                const float d_o = __shfl(d, (lane_id() & 48) | o, 64);
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (j0 + j < H / 16) dhv[j] = fmaf(d_o, w2v[o * (H + 1) + lo + 16 * (j0 + j)], dhv[j]);
            }
            if (ok) {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (j0 + j < H / 16) dh[row * H + lo + 16 * (j0 + j)] = hs[le * H + lo + 16 * (j0 + j)] > 0.0f ? dhv[j] : 0.0f;
            }
        }
    }
}

// policy(frames, action=...): the heads on GIVEN actions.  The softmax is eval_row16_heads (sampler.hpp, what the LSTM eval runs): its
// normalised logit is the expression sample_row16 forms, so the log-probability of an action cnn_heads_sample drew, and the value, come
// out as the same bits; the entropy is -sum nl p (the loss kernel's form).  The action is compared against the lane index, never indexed by.
template <int HT>
__global__ void __launch_bounds__(256) cnn_heads_eval_kernel(const float *h, int hrt, long long rows, CnnHeads hd, const long long *actions,
                                                            float *logprob, float *entropy, float *value) {
    extern __shared__ float lds[];
    const int H = HT ? HT : hrt;
    const CnnLds m{lds, H};
    float *w2v = m.w2v(), *b2v = m.b2v(), *hs = m.hs();
    cnn_stage_heads<HT>(hd, w2v, b2v, hrt);
    const int le = threadIdx.x >> 4, lo = threadIdx.x & 15, a = hd.a;
    const long long tiles = (rows + 15) / 16;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        cnn_stage_rows<HT>(h, hs, tile, rows, hrt);
        const long long row = tile * 16 + le;
        const bool ok = row < rows;
        const int action = ok ? (int)actions[row] : 0;
        const float mine = cnn_head_dot<HT>(hs + le * H, w2v, b2v, lo, hrt);
        const Row16Eval ev = eval_row16_heads(mine, lo, a, 0, action);
        const float v = row16_sum(lo == a ? mine : 0.0f);
        if (ok && lo == 0) {
            logprob[row] = ev.logprob;
            if (entropy) entropy[row] = ev.entropy;
            value[row] = v;
        }
    }
}

// Its backward for upstream gradients g_logprob / g_entropy / g_value [rows] (null = zero): the softmax recomputed by the forward's code
// from h alone, dout [rows][16] (columns < a: g_logprob (1[j = action] - p_j) - g_entropy p_j (nl_j + entropy), column a: g_value, the
// rest 0) and d / d (pre-ReLU hidden) [rows][H] with the loss kernel's mask and summation order.
template <int HT>
__global__ void __launch_bounds__(256) cnn_heads_eval_backward_kernel(const float *h, int hrt, long long rows, CnnHeads hd, const long long *actions,
                                                                     const float *g_logprob, const float *g_entropy, const float *g_value,
                                                                     float *dout /* [rows][16] */, float *dh /* [rows][H] */) {
    extern __shared__ float lds[];
    const int H = HT ? HT : hrt;
    const CnnLds m{lds, H};
    float *w2v = m.w2v(), *b2v = m.b2v(), *hs = m.hs();
    cnn_stage_heads<HT>(hd, w2v, b2v, hrt);
    const int le = threadIdx.x >> 4, lo = threadIdx.x & 15, a = hd.a;
    const long long tiles = (rows + 15) / 16;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        cnn_stage_rows<HT>(h, hs, tile, rows, hrt);
        const long long row = tile * 16 + le;
        const bool ok = row < rows;
        const int action = ok ? (int)actions[row] : 0;
        const float g_lp = ok && g_logprob ? g_logprob[row] : 0.0f;
        const float g_ent = ok && g_entropy ? g_entropy[row] : 0.0f;
        const float g_v = ok && g_value ? g_value[row] : 0.0f;
        const float mine = cnn_head_dot<HT>(hs + le * H, w2v, b2v, lo, hrt);
        const Row16Eval ev = eval_row16_heads(mine, lo, a, 0, action);
        float d = 0.0f;
        // (logit_grad with c_ent = -g_ent, kept as the subtraction it compiles to today: see heads_rows_eval_bwd_kernel, general.hip)
        if (ev.is_logit) d = g_lp * ((ev.chosen ? 1.0f : 0.0f) - ev.p) - g_ent * ev.p * (ev.nl + ev.head_entropy);
        else if (lo == a) d = g_v;
        if (ok) dout[row * kOut + lo] = d;
        cnn_heads_dh<HT>(d, w2v, hs, le, lo, a, ok, row, dh, hrt);
    }
}

// rows = a chunk [q0, q0 + rows) of minibatch `map.mb`; ex.* are read at map.flat(q0 + row).
template <int HT>
__global__ void __launch_bounds__(256) cnn_heads_loss_kernel(const float *h, int hrt, long long rows, RowMap map, long long q0, pfa_experience ex, CnnHeads hd,
                                                            pfa_ppo_hparams hp, const double *adv_stats, double global_rows,
                                                            float *dout /* [rows][16] */, float *dh /* [rows][H] */,
                                                            double *stats_partial /* [gridDim.x][8] */) {
    extern __shared__ float lds[];
    const int H = HT ? HT : hrt;
    const CnnLds m{lds, H};
    float *w2v = m.w2v(), *b2v = m.b2v(), *hs = m.hs();
    __shared__ double st[16][8];
    cnn_stage_heads<HT>(hd, w2v, b2v, hrt);
    const int le = threadIdx.x >> 4, lo = threadIdx.x & 15, a = hd.a;
    const AdvNorm norm = adv_norm(hp, adv_stats, map.mb, global_rows);
    const float inv_rows = (float)(1.0 / global_rows);
    double acc[6] = {0, 0, 0, 0, 0, 0};
    const long long tiles = (rows + 15) / 16;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        cnn_stage_rows<HT>(h, hs, tile, rows, hrt);
        const long long row = tile * 16 + le;
        const bool ok = row < rows;
        const long long fr = ok ? map.flat(q0 + row) : 0;
        const float w = ok ? 1.0f : 0.0f;
        const int action = ex.actions[fr];
        const float old_logprob = ex.logprobs[fr], old_value = ex.values[fr], adv_raw = ex.advantages[fr], ret = ex.returns[fr];
        const float mine = cnn_head_dot<HT>(hs + le * H, w2v, b2v, lo, hrt);
        // (the single-head case of eval_row16_heads(mine, lo, a, 0, action), expression for expression, spelled out: the call brings its
        // loop over heads along — ~50 more instructions per tile and other opcodes, docs/lab-notebook.md)
        const bool is_logit = lo < a;
        const float mx = row16_max(is_logit ? mine : -INFINITY);
        const float ev = is_logit ? expf(mine - mx) : 0.0f;
        const float se = row16_sum(ev);
        const float lse = mx + logf(se);
        const float nl = mine - lse, p = ev / se;
        const float ent = row16_sum(is_logit ? -nl * p : 0.0f);
        const bool chosen = lo == action;
        const float new_logprob = row16_sum(chosen ? nl : 0.0f);
        const float new_value = row16_sum(lo == a ? mine : 0.0f);
        const float scale = inv_rows * w;
        const float adv = hp.norm_adv ? (adv_raw - norm.mean) / norm.den : adv_raw;
        const PolicyLoss pl = ppo_policy_loss(new_logprob, old_logprob, adv, hp, scale);
        const ValueLoss vl = ppo_value_loss(new_value, old_value, ret, hp, scale);
        float d = 0.0f;
        if (is_logit) d = logit_grad(pl.g_lp, hp.ent_coef * scale, chosen, p, nl, ent);
        else if (lo == a) d = vl.dv;
        if (ok) dout[row * kOut + lo] = d;
        cnn_heads_dh<HT>(d, w2v, hs, le, lo, a, ok, row, dh, hrt);
        if (lo == 0) accumulate(acc, pl, vl, ent, hp, w);
    }
    __syncthreads();
    if (lo == 0)
        for (int i = 0; i < 8; ++i) st[le][i] = i < 6 ? acc[i] : 0.0;
    __syncthreads();
    if (threadIdx.x < 8) {
        double s = 0.0;
        for (int r = 0; r < 16; ++r) s += st[r][threadIdx.x];
        stats_partial[(size_t)blockIdx.x * 8 + threadIdx.x] = s;
    }
}

// loss_pairs16 (+)= the (hi, lo) pairs of the chunk's six sums (a minibatch is processed in chunks: accumulate != 0 adds)
__global__ void cnn_stats_final_kernel(const double *partial, int nblocks, float *loss_pairs16, int accumulate) {   // one wave
    const int i = threadIdx.x & 7, part = threadIdx.x >> 3;   // 8 sums x 8 interleaved block ranges
    double s = 0.0;
    for (int b = part; b < nblocks; b += 8) s += partial[(size_t)b * 8 + i];
    s += __shfl_xor(s, 8, 64);      // fixed combination order
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    if (threadIdx.x >= 8) return;
    if (accumulate) s += (double)loss_pairs16[2 * i] + (double)loss_pairs16[2 * i + 1];
    const float hi = (float)s;
    loss_pairs16[2 * i] = hi;
    loss_pairs16[2 * i + 1] = (float)(s - (double)hi);
}

// frames [B][frame_bytes] (env-major experience) -> out[rows][frame_bytes] for minibatch rows q0 .. q0 + rows - 1
__global__ void __launch_bounds__(256) cnn_gather_frames_kernel(const uint8_t *frames, long long frame_bytes, RowMap map, long long q0, long long rows,
                                                               uint8_t *out) {
    const long long per_row = frame_bytes / 16;   // 16-byte pieces
    const long long total = rows * per_row;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long r = i / per_row, c16 = i - r * per_row;
        const long long fr = map.flat(q0 + r);
        reinterpret_cast<uint4 *>(out + r * frame_bytes)[c16] = reinterpret_cast<const uint4 *>(frames + fr * frame_bytes)[c16];
    }
}

// the same for frames whose size is not a multiple of 16 bytes (odd frame shapes such as 9 x 7 x 3): byte by byte
__global__ void __launch_bounds__(256) cnn_gather_frames_bytes_kernel(const uint8_t *frames, long long frame_bytes, RowMap map, long long q0, long long rows,
                                                                     uint8_t *out) {
    const long long total = rows * frame_bytes;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long r = i / frame_bytes, c = i - r * frame_bytes;
        out[i] = frames[map.flat(q0 + r) * frame_bytes + c];
    }
}

static size_t cnn_heads_lds(int H) { return (size_t)(kOut * (H + 1) + kOut + 16 * H) * sizeof(float); }

// Launch of heads kernel K (any of the four, any width instantiation: K(h, H, args...)) with the dynamic LDS of hidden width H.
// lds_set: the opt-in LDS size of THIS instantiation so far (it grows with the run-time width).
template <auto K, class... Args>
static int cnn_launch(int H, unsigned grid, hipStream_t stream, const float *h, Args... args) {
    static int lds_set = 0;
    const int lds = (int)cnn_heads_lds(H);
    if (lds > lds_set) {
        PFA_CHECK_HIP(hipFuncSetAttribute((const void *)K, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        lds_set = lds;
    }
    hipLaunchKernelGGL(K, dim3(grid), dim3(256), lds, stream, h, H, args...);
    PFA_LAUNCH_CHECK();
    return 0;
}

// f(std::integral_constant<int, HT>) for the instantiation that runs hidden width `hidden`: 512, 128, or 0 = the run-time-width code
template <class F>
static int cnn_hidden(int hidden, F &&f) {
    if (hidden == 512) return f(std::integral_constant<int, 512>{});
    if (hidden == 128) return f(std::integral_constant<int, 128>{});
    return f(std::integral_constant<int, 0>{});
}

}  // namespace pfa

using namespace pfa;

extern "C" int pfa_cnn_heads_sample(const float *h, int32_t hidden, int64_t rows, const float *actor_w, const float *actor_b, const float *value_w,
                                    const float *value_b, int32_t num_actions, const float *noise, const pfa_noise_key *key, int64_t row_offset,
                                    int64_t *actions, float *logprob, float *entropy, float *value, pfa_stream_t stream) {
    PFA_REQUIRE(rows >= 0 && h && actor_w && actor_b && value_w && value_b && actions && logprob && value, "cnn.heads_sample: null buffer");
    PFA_REQUIRE(hidden >= 16 && hidden % 16 == 0 && hidden <= kCnnMaxH, "cnn.heads_sample: hidden must be a multiple of 16 in 16..1024 (got %d)", hidden);
    PFA_REQUIRE(num_actions >= 1 && num_actions <= 15, "cnn.heads_sample: num_actions must be in 1..15");
    PFA_REQUIRE(noise || key, "cnn.heads_sample: need an explicit noise tensor or a Philox key");
    if (rows == 0) return 0;
    const long long tiles = (rows + 15) / 16;
    const unsigned grid = (unsigned)(tiles < 1024 ? tiles : 1024);
    CnnHeads hd{actor_w, actor_b, value_w, value_b, (int)num_actions};
    ScopedKernelTimer timer("cnn_heads_sample", (hipStream_t)stream);
    return cnn_hidden(hidden, [&](auto ht) {
        return cnn_launch<cnn_heads_sample_kernel<decltype(ht)::value>>((int)hidden, grid, (hipStream_t)stream, h, (long long)rows, hd, noise,
                                                                        key ? key->seed : 0, key ? key->step : 0, (long long)row_offset,
                                                                        (long long *)actions, logprob, entropy, value);
    });
}

extern "C" int pfa_cnn_heads_eval(const float *h, int32_t hidden, int64_t rows, const float *actor_w, const float *actor_b, const float *value_w,
                                  const float *value_b, int32_t num_actions, const int64_t *actions, float *logprob, float *entropy, float *value,
                                  pfa_stream_t stream) {
    PFA_REQUIRE(rows >= 0 && h && actor_w && actor_b && value_w && value_b && actions && logprob && value, "cnn.heads_eval: null buffer");
    PFA_REQUIRE(hidden >= 16 && hidden % 16 == 0 && hidden <= kCnnMaxH, "cnn.heads_eval: hidden must be a multiple of 16 in 16..1024 (got %d)", hidden);
    PFA_REQUIRE(num_actions >= 1 && num_actions <= 15, "cnn.heads_eval: num_actions must be in 1..15");
    if (rows == 0) return 0;
    const long long tiles = (rows + 15) / 16;
    const unsigned grid = (unsigned)(tiles < 1024 ? tiles : 1024);
    CnnHeads hd{actor_w, actor_b, value_w, value_b, (int)num_actions};
    ScopedKernelTimer timer("cnn_heads_eval", (hipStream_t)stream);
    return cnn_hidden(hidden, [&](auto ht) {
        return cnn_launch<cnn_heads_eval_kernel<decltype(ht)::value>>((int)hidden, grid, (hipStream_t)stream, h, (long long)rows, hd,
                                                                      (const long long *)actions, logprob, entropy, value);
    });
}

extern "C" int pfa_cnn_heads_eval_backward(const float *h, int32_t hidden, int64_t rows, const float *actor_w, const float *actor_b,
                                           const float *value_w, const float *value_b, int32_t num_actions, const int64_t *actions,
                                           const float *g_logprob, const float *g_entropy, const float *g_value, float *dout, float *dh,
                                           pfa_stream_t stream) {
    PFA_REQUIRE(rows >= 0 && h && actor_w && actor_b && value_w && value_b && actions && dout && dh, "cnn.heads_eval_backward: null buffer");
    PFA_REQUIRE(hidden >= 16 && hidden % 16 == 0 && hidden <= kCnnMaxH, "cnn.heads_eval_backward: hidden must be a multiple of 16 in 16..1024 (got %d)", hidden);
    PFA_REQUIRE(num_actions >= 1 && num_actions <= 15, "cnn.heads_eval_backward: num_actions must be in 1..15");
    if (rows == 0) return 0;
    const long long tiles = (rows + 15) / 16;
    const unsigned grid = (unsigned)(tiles < 1024 ? tiles : 1024);
    CnnHeads hd{actor_w, actor_b, value_w, value_b, (int)num_actions};
    ScopedKernelTimer timer("cnn_heads_eval_backward", (hipStream_t)stream);
    return cnn_hidden(hidden, [&](auto ht) {
        return cnn_launch<cnn_heads_eval_backward_kernel<decltype(ht)::value>>((int)hidden, grid, (hipStream_t)stream, h, (long long)rows, hd,
                                                                               (const long long *)actions, g_logprob, g_entropy, g_value, dout, dh);
    });
}

extern "C" size_t pfa_cnn_heads_loss_workspace_bytes(void) { return (size_t)1024 * 8 * sizeof(double); }

extern "C" int pfa_cnn_heads_loss(const float *h, int32_t hidden, const pfa_experience *exp, int64_t batch_rows, int32_t mb, int64_t q0, int64_t rows,
                                  const float *actor_w, const float *actor_b, const float *value_w, const float *value_b, int32_t num_actions,
                                  const pfa_ppo_hparams *hp, const double *adv_stats, int64_t global_mb_rows, float *dout, float *dh,
                                  float *loss_pairs16, int32_t accumulate, void *workspace, pfa_stream_t stream) {
    PFA_REQUIRE(h && exp && hp && dout && dh && loss_pairs16 && workspace && actor_w && actor_b && value_w && value_b, "cnn.heads_loss: null buffer");
    PFA_REQUIRE(num_actions >= 1 && num_actions <= 15, "cnn.heads_loss: num_actions must be in 1..15");
    PFA_REQUIRE(hidden >= 16 && hidden % 16 == 0 && hidden <= kCnnMaxH, "cnn.heads_loss: hidden must be a multiple of 16 in 16..1024 (got %d)", hidden);
    PFA_REQUIRE(hp->num_minibatches >= 1 && batch_rows % hp->num_minibatches == 0 && mb >= 0 && mb < hp->num_minibatches, "cnn.heads_loss: bad minibatch");
    const int64_t mbs = batch_rows / hp->num_minibatches;
    PFA_REQUIRE(q0 >= 0 && rows >= 1 && q0 + rows <= mbs, "cnn.heads_loss: chunk outside the minibatch");
    PFA_REQUIRE(!hp->norm_adv || adv_stats, "cnn.heads_loss: norm_adv needs adv_stats");
    const long long tiles = (rows + 15) / 16;
    const unsigned grid = (unsigned)(tiles < 1024 ? tiles : 1024);
    CnnHeads hd{actor_w, actor_b, value_w, value_b, (int)num_actions};
    RowMap map{mb, hp->num_minibatches, hp->bptt_horizon};
    ScopedKernelTimer timer("cnn_heads_loss", (hipStream_t)stream);
    const int rc = cnn_hidden(hidden, [&](auto ht) {
        return cnn_launch<cnn_heads_loss_kernel<decltype(ht)::value>>((int)hidden, grid, (hipStream_t)stream, h, (long long)rows, map, (long long)q0, *exp,
                                                                      hd, *hp, adv_stats, (double)global_mb_rows, dout, dh, (double *)workspace);
    });
    if (rc) return rc;
    hipLaunchKernelGGL(cnn_stats_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double *)workspace, (int)grid, loss_pairs16, (int)accumulate);
    PFA_LAUNCH_CHECK();
    return 0;
}

extern "C" int pfa_cnn_gather_frames(const uint8_t *frames, int64_t frame_bytes, int64_t batch_rows, int32_t mb, const pfa_ppo_hparams *hp,
                                     int64_t q0, int64_t rows, uint8_t *out, pfa_stream_t stream) {
    PFA_REQUIRE(frames && out && hp && frame_bytes >= 1, "cnn.gather_frames: null buffer or empty frames");
    PFA_REQUIRE(hp->num_minibatches >= 1 && batch_rows % hp->num_minibatches == 0 && mb >= 0 && mb < hp->num_minibatches, "cnn.gather_frames: bad minibatch");
    PFA_REQUIRE(q0 >= 0 && rows >= 1 && q0 + rows <= batch_rows / hp->num_minibatches, "cnn.gather_frames: chunk outside the minibatch");
    RowMap map{mb, hp->num_minibatches, hp->bptt_horizon};
    if (frame_bytes % 16 != 0) {
        const long long bytes = rows * frame_bytes;
        const unsigned g = (unsigned)((bytes + 255) / 256 < 65535 ? (bytes + 255) / 256 : 65535);
        hipLaunchKernelGGL(cnn_gather_frames_bytes_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, frames, (long long)frame_bytes, map, (long long)q0,
                           (long long)rows, out);
        PFA_LAUNCH_CHECK();
        return 0;
    }
    const long long total = rows * (frame_bytes / 16);
    const unsigned grid = (unsigned)((total + 255) / 256 < 65535 ? (total + 255) / 256 : 65535);
    hipLaunchKernelGGL(cnn_gather_frames_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, frames, (long long)frame_bytes, map, (long long)q0,
                       (long long)rows, out);
    PFA_LAUNCH_CHECK();
    return 0;
}
