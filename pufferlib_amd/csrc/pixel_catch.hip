// pixel_catch.hip — the PixelCatch vecenv: the Catch state machine of catch_env.hpp shown as uint8 frames whose channels are a time
// stack — channel k shows the state framestack-1-k sends ago (history slot framestack-1-k), oldest first — in (C, H, W) or (H, W, C)
// order.  Pixel (y, x) shows cell (y*rows / H, x*cols / W); the ball's cell is 255, the paddle's 128, every other 0.
//
// One launch per send (and per reset), two phases in a workgroup that owns `epw` consecutive envs (the last workgroup possibly fewer):
//   step    lane k < envs owned: catch_send (or the first episode's start) on env k, then the env's slots into LDS as one word each:
//           ball cell | paddle cell << 16, a cell being row * cols + column
//   paint   the frame is cut into 16-byte chunks, consecutive lanes on consecutive chunks, every chunk written with one 16-byte
//           store.  A frame has two kinds of cell that are not 0, so nothing is looked up per byte: a lane works out ONCE per chunk,
//           for all owned envs, the cell each of its 16 bytes shows (two tables built per launch: pixel row -> cell row * cols, pixel
//           column -> cell column; the (outer, middle, inner) position of its next chunk by adding the digits of the stride: no
//           division per byte) and which slots the chunk shows; per env it then reads those slots' words — in channel-first one word
//           (two where the chunk crosses into the next channel, which happens only when H * W is no multiple of 16: that form is its
//           own instantiation), in channel-last `framestack` words, rotated by the chunk's first channel so that byte k always
//           compares with word k % C — and every byte is two compares and two selects on registers.
// Roofline: framestack * H * W bytes written per env and send (28 KB at (4, 84, 84): 231 MB at 8192 envs), 88 B of state touched:
// HBM-write bound.
#include "common.hpp"
#include "env_adapters.hpp"
#include "catch_env.hpp"

namespace pfa {

constexpr int kCatchThreads = 256;
constexpr int kCatchMaxEnvs = 8;      // envs per workgroup, at most
constexpr int kCatchChunk = 16;
constexpr uint32_t kCatchBall = 255, kCatchPaddle = 128;

struct CatchPaint {
    int height, width;
    int chunks;           // 16-byte chunks per frame
    int epw;              // envs per workgroup
    int st0, st1, st2;    // (outer, middle, inner) digits of the kCatchThreads * 16 bytes between a lane's chunks
};

// The 16 cells of the chunk that starts at position (a0, a1, a2) — (y, x, c) channel-last, (c, y, x) channel-first —, the slots
// its words come from and, channel-first, the first byte of the next channel (16: the chunk stays in one).
template <int C, bool CL>
__device__ __forceinline__ void catch_chunk(const CatchPaint &p, const uint16_t *ytab, const uint16_t *xtab, int a0, int a1, int a2,
                                            uint32_t (&cell)[kCatchChunk], int (&slot)[CL ? C : 2], int &kb) {
    kb = kCatchChunk;
    if constexpr (CL) {
        int y = a0, x = a1, c = a2;
        uint32_t cur = (uint32_t)ytab[y] + xtab[x];
#pragma unroll
        for (int k = 0; k < kCatchChunk; ++k) {
            cell[k] = cur;
            if (++c == C) {
                c = 0;
                if (++x == p.width) {
                    x = 0;
                    ++y;           // == height only behind the frame's last byte: the tables have a spare entry
                }
                cur = (uint32_t)ytab[y] + xtab[x];
            }
        }
#pragma unroll
        for (int i = 0; i < C; ++i) {
            const int ch = a2 + i < C ? a2 + i : a2 + i - C;     // byte k shows channel (a2 + k) % C = that of word k % C
            slot[i] = C - 1 - ch;
        }
    } else {
        int y = a1, x = a2;
        uint32_t row = ytab[y];
#pragma unroll
        for (int k = 0; k < kCatchChunk; ++k) {
            cell[k] = row + xtab[x];
            if (++x == p.width) {
                x = 0;
                if (++y == p.height) {
                    y = 0;
                    // One crossing per chunk: C * H * W is a multiple of 16 with C <= kCatchStack = 4, so H * W is a multiple of 4,
                    // and the smallest frames (H * W = 8, 12) start their chunks where a second crossing cannot fall inside one.
                    // A relaxed 16-byte rule or a larger kCatchStack breaks this: catch_launch requires it.
                    if (kb == kCatchChunk && k < kCatchChunk - 1) kb = k + 1;
                }
                row = ytab[y];
            }
        }
        slot[0] = C - 1 - a0;
        slot[1] = a0 + 1 < C ? C - 2 - a0 : 0;
    }
}

// actions == nullptr: the reset (every env begins episode 0) and its frames
template <int C, bool CL, bool STRADDLE>
__global__ void __launch_bounds__(kCatchThreads) pixel_catch_kernel(CatchView v, CatchPaint p, const long long *actions, uint8_t *obs,
                                                                    float *rewards, uint8_t *terminals, uint8_t *truncations,
                                                                    uint8_t *masks) {
    __shared__ uint16_t s_ytab[kCatchMaxSide + 1], s_xtab[kCatchMaxSide + 1];   // pixel row -> cell row * cols; pixel column -> cell column
    __shared__ uint32_t s_bp[kCatchMaxEnvs][kCatchStack];                       // [env][slot] ball cell | paddle cell << 16
    const int tid = threadIdx.x;
    const int e0 = blockIdx.x * p.epw;
    const int owned = v.n - e0 < p.epw ? v.n - e0 : p.epw;     // tail workgroup: fewer envs

    if (tid < owned) {
        const int e = e0 + tid;
        CatchRollEnv env;
        float reward = 0.0f;
        bool terminal = false;
        if (actions == nullptr) {
            env.reset(v, e);
        } else {
            env.load(v, e);
            env.step(v, e, (int)actions[e], reward, terminal);
        }
        env.store(v, e);
#pragma unroll
        for (int j = 0; j < kCatchStack; ++j)
            s_bp[tid][j] = (uint32_t)(env.s.r[j] * v.cols + env.s.c[j]) | ((uint32_t)((v.rows - 1) * v.cols + env.s.p[j]) << 16);
        rewards[e] = reward;
        terminals[e] = terminal ? 1 : 0;
        truncations[e] = 0;
        masks[e] = 1;
    }
    for (int y = tid; y <= p.height; y += kCatchThreads) s_ytab[y] = (uint16_t)(y < p.height ? (y * v.rows / p.height) * v.cols : 0);
    for (int x = tid; x <= p.width; x += kCatchThreads) s_xtab[x] = (uint16_t)(x < p.width ? x * v.cols / p.width : 0);
    __syncthreads();

    const int d1 = CL ? p.width : p.height, d2 = CL ? C : p.width;
    int a2 = (tid * kCatchChunk) % d2, t = (tid * kCatchChunk) / d2;   // this lane's first chunk: the only divisions of the paint phase
    int a1 = t % d1, a0 = t / d1;
    const size_t frame_bytes = (size_t)p.chunks * kCatchChunk;
    uint8_t *out = obs + (size_t)e0 * frame_bytes;
    constexpr int NW = CL ? C : 2;
    for (int q = tid; q < p.chunks; q += kCatchThreads) {
        uint32_t cell[kCatchChunk];
        int slot[NW], kb;
        catch_chunk<C, CL>(p, s_ytab, s_xtab, a0, a1, a2, cell, slot, kb);
        for (int le = 0; le < owned; ++le) {
            uint32_t ball[NW], pad[NW];
#pragma unroll
            for (int i = 0; i < (CL || STRADDLE ? NW : 1); ++i) {
                const uint32_t bp = s_bp[le][slot[i]];
                ball[i] = bp & 0xffffu;
                pad[i] = bp >> 16;
            }
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < kCatchChunk; ++k) {
                uint32_t b, d;
                if constexpr (CL) {
                    b = ball[k % C], d = pad[k % C];
                } else if constexpr (STRADDLE) {
                    b = k < kb ? ball[0] : ball[1], d = k < kb ? pad[0] : pad[1];
                } else {
                    b = ball[0], d = pad[0];
                }
                uint32_t byte = cell[k] == d ? kCatchPaddle : 0u;
                byte = cell[k] == b ? kCatchBall : byte;          // the ball wins where both are
                w[k / 4] = k % 4 == 0 ? byte : w[k / 4] | (byte << (8 * (k % 4)));
            }
            *reinterpret_cast<uint4 *>(out + (size_t)le * frame_bytes + (size_t)q * kCatchChunk) = make_uint4(w[0], w[1], w[2], w[3]);
        }
        a2 += p.st2;     // digits of the next chunk: each sum stays below twice its dim, one carry each
        if (a2 >= d2) { a2 -= d2; a1 += 1; }
        a1 += p.st1;
        if (a1 >= d1) { a1 -= d1; a0 += 1; }
        a0 += p.st0;
    }
}

__global__ void __launch_bounds__(256) pixel_catch_debug_states_kernel(CatchView v, int32_t *out16) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= v.n) return;
    const CatchEnv s = v.env[e];
    int32_t *o = out16 + (size_t)e * 16;
    for (int j = 0; j < kCatchStack; ++j) o[3 * j] = s.r[j], o[3 * j + 1] = s.c[j], o[3 * j + 2] = s.p[j];
    o[12] = s.vx, o[13] = s.episode, o[14] = s.ep_length, o[15] = 0;
}

// Envs per workgroup, by the rule pixel_squared.hip measured for the same shape of kernel: what a workgroup does before it paints (the
// tables, the barrier, a lane's first position) and per chunk (the 16 cells) costs the same for one env as for eight, so it owns as
// many as still leave every CU four workgroups.
static int catch_envs_per_wg(int num_envs) {
    int epw = 1;
    while (epw < kCatchMaxEnvs && num_envs / (2 * epw) >= 1024) epw *= 2;
    return epw;
}

template <int C, bool CL, bool STRADDLE>
static void catch_launch_as(const CatchView &v, const CatchPaint &p, const int64_t *actions, uint8_t *obs, float *rewards, uint8_t *terminals,
                            uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    const unsigned blocks = (unsigned)((v.n + p.epw - 1) / p.epw);
    hipLaunchKernelGGL((pixel_catch_kernel<C, CL, STRADDLE>), dim3(blocks), dim3(kCatchThreads), 0, (hipStream_t)stream, v, p,
                       (const long long *)actions, obs, rewards, terminals, truncations, masks);
}

static int catch_launch(const char *what, void *state, const pfa_pixel_catch_config *cfg, const int64_t *actions, uint8_t *obs, float *rewards,
                        uint8_t *terminals, uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    if (int rc = CatchRollEnv::check(cfg)) return rc;
    PFA_REQUIRE(state && obs && rewards && terminals && truncations && masks, "pixel_catch.%s: null buffer", what);
    const CatchView v = CatchRollEnv::view(state, *cfg);
    const int C = cfg->framestack;
    const bool cl = cfg->channels_last != 0 || C == 1;     // (one channel: both orders are the same bytes)
    const bool straddle = !cl && (cfg->height * cfg->width) % kCatchChunk != 0;
    static_assert(kCatchStack <= 4, "the crossing form of the painter counts on one channel border per chunk");
    PFA_REQUIRE(!straddle || ((cfg->height * cfg->width) % 4 == 0 && cfg->height * cfg->width >= 8),
                "pixel_catch.%s: channels of %d bytes would cross a 16-byte chunk twice", what, cfg->height * cfg->width);
    CatchPaint p;
    p.height = cfg->height;
    p.width = cfg->width;
    p.chunks = cfg->height * cfg->width * C / kCatchChunk;
    p.epw = catch_envs_per_wg(cfg->num_envs);
    const int d1 = cl ? cfg->width : cfg->height, d2 = cl ? C : cfg->width, step = kCatchThreads * kCatchChunk;
    p.st2 = step % d2;
    p.st1 = step / d2 % d1;
    p.st0 = step / d2 / d1;
#define PFA_CATCH_CASE(C)                                                                                                     \
    case C:                                                                                                                   \
        if (cl) catch_launch_as<C, true, false>(v, p, actions, obs, rewards, terminals, truncations, masks, stream);          \
        else if (straddle) catch_launch_as<C, false, true>(v, p, actions, obs, rewards, terminals, truncations, masks, stream); \
        else catch_launch_as<C, false, false>(v, p, actions, obs, rewards, terminals, truncations, masks, stream);            \
        break;
    switch (C) {
        PFA_CATCH_CASE(1)
        PFA_CATCH_CASE(2)
        PFA_CATCH_CASE(3)
        PFA_CATCH_CASE(4)
    }
#undef PFA_CATCH_CASE
    PFA_LAUNCH_CHECK();
    return 0;
}

}  // namespace pfa

using namespace pfa;

extern "C" size_t pfa_pixel_catch_state_bytes(const pfa_pixel_catch_config *cfg) { return env_state_bytes<CatchRollEnv>(cfg); }

extern "C" int pfa_pixel_catch_async_reset(void *state, const pfa_pixel_catch_config *cfg, uint8_t *obs, float *rewards, uint8_t *terminals,
                                           uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    return catch_launch("async_reset", state, cfg, nullptr, obs, rewards, terminals, truncations, masks, stream);
}

extern "C" int pfa_pixel_catch_send(void *state, const pfa_pixel_catch_config *cfg, const int64_t *actions, uint8_t *obs, float *rewards,
                                    uint8_t *terminals, uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    PFA_REQUIRE(actions, "pixel_catch.send: null buffer");
    return catch_launch("send", state, cfg, actions, obs, rewards, terminals, truncations, masks, stream);
}

extern "C" int pfa_pixel_catch_episode_stats(void *state, const pfa_pixel_catch_config *cfg, double *out4, int32_t reset, pfa_stream_t stream) {
    return env_episode_stats<CatchRollEnv>(state, cfg, out4, reset, stream);
}

extern "C" int pfa_pixel_catch_last_infos(void *state, const pfa_pixel_catch_config *cfg, uint8_t *finished, double *episode_return,
                                          int32_t *episode_length, double *score, pfa_stream_t stream) {
    return env_last_infos<CatchRollEnv>(state, cfg, finished, episode_return, episode_length, score, stream);
}

extern "C" int pfa_pixel_catch_debug_states(void *state, const pfa_pixel_catch_config *cfg, int32_t *out16, pfa_stream_t stream) {
    if (int rc = CatchRollEnv::check(cfg)) return rc;
    PFA_REQUIRE(state && out16, "pixel_catch.debug_states: null buffer");
    return launch_per_env(pixel_catch_debug_states_kernel, cfg->num_envs, stream, CatchRollEnv::view(state, *cfg), out16);
}
