// catch_env.hpp — Catch: a ball falls diagonally through a rows x cols grid, one row per send, and a paddle on the bottom row must be
// under it when it lands.  Integer dynamics only.  Per env the state is the last kCatchStack (ball row, ball column, paddle column)
// triples — slot 0 the current one, slot j the one j sends ago, never older than the episode's start state — and {vx, episode,
// ep_length, f64 ep_return} next to an EpisodeFin.  pixel_catch.hip paints the slots as the channels of a time stack of frames; a
// flat-row family on the fused rollout skeletons would read slot 0 (catch_send is what its adapter's step would call).
//
// One send:
//   paddle   p' = clamp(p + action - 1, 0, cols - 1)                      (actions: 0 left, 1 stay, 2 right; others are clamped)
//   ball     c' = c + vx; where c' leaves [0, cols - 1]: vx = -vx, c' = c + vx;   r' = r + 1
//   r' == rows - 1: the episode ends — reward +1 when c' == p', else -1, terminal, the episode is accounted (score 1 / 0, length
//            rows - 1, return = the reward) — and the next one begins inside the same send: every slot holds its start state, which
//            is what the observation of the terminal row shows.  There is no auto-reset row: every send takes its action.
//   else     reward 0
// Randomness is counter-based, there is no tape: the start state of (env, episode) is
//   ball column w0 % cols, vx = w1 % 3 - 1, paddle column w2 % cols, ball row 0,
//   (w0, w1, w2, _) = Philox4x32-10(counter = (global env, episode, 0, 0), key = (seed lo, 'PC' ^ seed hi))
#pragma once
#include "common.hpp"
#include "episode_fin.hpp"
#include "philox.hpp"

namespace pfa {

constexpr int kCatchStack = 4;        // history slots kept per env = the largest framestack
constexpr int kCatchMaxSide = 1024;   // height, width of a frame: entries of the painter's two tables

struct CatchEnv {
    uint16_t r[kCatchStack], c[kCatchStack], p[kCatchStack];
    int vx, episode, ep_length, pad;
    double ep_return;
};
struct CatchView {
    CatchEnv *env;
    EpisodeFin *fin;
    int n, rows, cols;
    uint32_t key0, key1;
    long long env_offset;
};

__device__ __forceinline__ void catch_begin_episode(const CatchView &v, int e, CatchEnv &s) {
    s.episode += 1;
    s.ep_length = 0;
    s.ep_return = 0.0;
    const u32x4 w = philox4x32_10((uint32_t)(v.env_offset + e), (uint32_t)s.episode, 0u, 0u, v.key0, v.key1);
    s.vx = (int)(w.y % 3u) - 1;
#pragma unroll
    for (int j = 0; j < kCatchStack; ++j) {
        s.r[j] = 0;
        s.c[j] = (uint16_t)(w.x % (uint32_t)v.cols);
        s.p[j] = (uint16_t)(w.z % (uint32_t)v.cols);
    }
}

// one send of env e; returns true when it finished (and accounted) an episode
__device__ __forceinline__ bool catch_send(const CatchView &v, int e, CatchEnv &s, int action, float &reward, bool &terminal) {
    const int p = min(max((int)s.p[0] + min(max(action, 0), 2) - 1, 0), v.cols - 1);
    int c = (int)s.c[0] + s.vx;
    if (c < 0 || c >= v.cols) {
        s.vx = -s.vx;
        c = (int)s.c[0] + s.vx;
    }
    const int r = (int)s.r[0] + 1;
#pragma unroll
    for (int j = kCatchStack - 1; j > 0; --j) s.r[j] = s.r[j - 1], s.c[j] = s.c[j - 1], s.p[j] = s.p[j - 1];
    s.r[0] = (uint16_t)r, s.c[0] = (uint16_t)c, s.p[0] = (uint16_t)p;
    s.ep_length += 1;
    terminal = r == v.rows - 1;
    reward = 0.0f;
    if (terminal) {
        reward = c == p ? 1.0f : -1.0f;
        s.ep_return += (double)reward;
        episode_account(v.fin[e], s.ep_return, s.ep_length, c == p ? 1.0 : 0.0);
        catch_begin_episode(v, e, s);
    }
    return terminal;
}

// What the protocol front (env_adapters.hpp: env_state_bytes, env_episode_stats, env_last_infos) asks of a family, and the owner
// thread's load / reset / step / store for the painter's kernel.  It is NOT an adapter of env_adapters.hpp: the observation is no
// float row, so these take no (lane, Shared, row) and there is no Shared, kRefresh or stride(); env_send_kernel and the fused rollouts
// cannot take this struct.  A flat-row family would wrap catch_send in an adapter of its own.
struct CatchRollEnv {
    using View = CatchView;
    using Config = pfa_pixel_catch_config;
    static constexpr const char *kName = "pixel_catch";
    CatchEnv s = {};
    int last_fin = 0;

    static int check(const Config *c) {
        PFA_REQUIRE(c != nullptr, "pixel_catch: null config");
        PFA_REQUIRE(c->num_envs >= 1, "pixel_catch: num_envs must be >= 1 (got %d)", c->num_envs);
        PFA_REQUIRE(c->rows >= 3 && c->cols >= 2, "pixel_catch: the grid must have at least 3 rows and 2 columns (got %d x %d)", c->rows, c->cols);
        PFA_REQUIRE((long long)c->rows * c->cols <= 65536, "pixel_catch: the grid must have at most 65536 cells (got %d x %d)", c->rows, c->cols);
        PFA_REQUIRE(c->height >= c->rows && c->width >= c->cols && c->height <= kCatchMaxSide && c->width <= kCatchMaxSide,
                    "pixel_catch: height must be in %d..%d and width in %d..%d (one pixel per grid cell at least), got %d x %d", c->rows,
                    kCatchMaxSide, c->cols, kCatchMaxSide, c->height, c->width);
        PFA_REQUIRE(c->framestack >= 1 && c->framestack <= kCatchStack, "pixel_catch: framestack must be in 1..%d (got %d)", kCatchStack,
                    c->framestack);
        PFA_REQUIRE((c->height * c->width * c->framestack) % 16 == 0,
                    "pixel_catch: frames are written in 16-byte chunks, %d x %d x %d bytes is no multiple", c->framestack, c->height, c->width);
        return 0;
    }
    static size_t state_bytes(int n) { return (size_t)n * (sizeof(CatchEnv) + sizeof(EpisodeFin)); }
    static View view(void *state, const Config &c) {
        View v;
        v.env = (CatchEnv *)state;
        v.fin = (EpisodeFin *)((char *)state + (size_t)c.num_envs * sizeof(CatchEnv));
        v.n = c.num_envs;
        v.rows = c.rows;
        v.cols = c.cols;
        v.key0 = (uint32_t)c.seed;
        v.key1 = 0x5043u ^ (uint32_t)(c.seed >> 32);   // 'PC'
        v.env_offset = c.env_offset;
        return v;
    }

    __device__ __forceinline__ void load(const View &v, int e) { s = v.env[e]; }
    __device__ __forceinline__ void reset(const View &v, int e) {
        s = CatchEnv{};
        s.episode = -1;
        catch_begin_episode(v, e, s);
        v.fin[e] = EpisodeFin{};
        last_fin = 0;
    }
    __device__ __forceinline__ void step(const View &v, int e, int action, float &reward, bool &terminal) {
        last_fin = catch_send(v, e, s, action, reward, terminal) ? 1 : 0;
    }
    __device__ __forceinline__ void store(const View &v, int e) {
        v.env[e] = s;
        v.fin[e].last_fin = last_fin;
    }
};

}  // namespace pfa
