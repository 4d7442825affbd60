// tabular_env.hpp — a user-given finite MDP / POMDP as device tables (vector.TabularMDP -> pfa_tabular_config): one env family
// that walks them.  Per env the state is {state index, episode, tick, done, ep_length, f64 ep_return} next to an EpisodeFin.
//
// One send (vector.py:137-156 of the reference: Serial's protocol; the send after a terminal row is the auto-reset row):
//   done       action ignored, reward 0, terminal false, episode += 1, tick = 0, a start state is drawn
//   otherwise  outcome k of (state, action) is drawn; state' = next[s][a][k]; reward = (float)reward[s][a][k] (f64 table, summed as
//              f64 into the episode return in order, like EpisodeStats); tick += 1; terminal = terminal[state'] || tick == horizon;
//              on terminal the episode is accounted with score = score[state'] (no score table: the episode's return)
// The observation row is obs[state'], `obs_stride` floats, zero-padded behind the obs_dim real values.
//
// Randomness is counter-based, there is no tape:
//   word = Philox4x32-10(counter = (global env, episode, tick, domain), key = (seed lo, 'TB' ^ seed hi)).x
// domain 0 = the start draw (tick 0), 1 = a transition; tick = steps already taken in the episode.  Probabilities were turned into
// uint32 thresholds on the host (vector.TabularMDP: cum[k] = floor(2^32 * sum_{j<=k} prob_j) clipped to 2^32 - 1), and
//   outcome = number of j with cum[j] <= min(word, cum[last] - 1)
// = the first k with word < cum[k], else — word >= cum[last], which only rounding makes possible — the last outcome whose threshold
// rises above its predecessor's (the last one with non-zero probability at this resolution).  An outcome with cum[k] == cum[k-1] is
// never drawn.  A table with one outcome per (state, action) / one start state draws nothing (wave-uniform flags in the view): the
// ten Philox rounds otherwise sit on the fused rollouts' per-step dependent chain.
#pragma once
#include "common.hpp"
#include "episode_fin.hpp"
#include "philox.hpp"

namespace pfa {

constexpr int kTabMaxStates = 1 << 20, kTabMaxActions = 1024, kTabMaxOutcomes = 8, kTabMaxObs = 160;

struct TabularEnv {
    int state, episode, tick, done, ep_length;
    double ep_return;
};
struct TabularView {
    TabularEnv *env;
    EpisodeFin *fin;
    int n, S, A, K, M, stride, horizon;
    bool draw_k, draw_m;     // K > 1 / M > 1: wave-uniform, so a deterministic table never enters the Philox rounds
    uint32_t key0, key1;
    long long env_offset;
    const int32_t *next;
    const uint32_t *cum;
    const double *reward;
    const uint8_t *terminal;
    const double *score;     // nullable
    const float *obs;
    const int32_t *start_states;
    const uint32_t *start_cum;
};
__host__ __device__ inline size_t tabular_state_bytes(int n) { return (size_t)n * (sizeof(TabularEnv) + sizeof(EpisodeFin)); }
__host__ __device__ inline TabularView tabular_view(void *state, const pfa_tabular_config &c) {
    TabularView v;
    v.env = (TabularEnv *)state;
    v.fin = (EpisodeFin *)((char *)state + (size_t)c.num_envs * sizeof(TabularEnv));
    v.n = c.num_envs;
    v.S = c.num_states;
    v.A = c.num_actions;
    v.K = c.num_outcomes;
    v.M = c.num_starts;
    v.stride = c.obs_stride;
    v.horizon = c.horizon;
    v.draw_k = c.num_outcomes > 1;
    v.draw_m = c.num_starts > 1;
    v.key0 = (uint32_t)c.seed;
    v.key1 = 0x5442u ^ (uint32_t)(c.seed >> 32);
    v.env_offset = c.env_offset;
    v.next = c.next;
    v.cum = c.cum;
    v.reward = c.reward;
    v.terminal = c.terminal;
    v.score = c.score;
    v.obs = c.obs;
    v.start_states = c.start_states;
    v.start_cum = c.start_cum;
    return v;
}

__device__ __forceinline__ uint32_t tabular_word(const TabularView &v, int e, int episode, int tick, uint32_t domain) {
    return philox4x32_10((uint32_t)(v.env_offset + e), (uint32_t)episode, (uint32_t)tick, domain, v.key0, v.key1).x;
}

// the start state of (env, episode): binary search of the M thresholds (M <= 2^20: at most 20 dependent reads, once per episode)
__device__ __forceinline__ int tabular_draw_start(const TabularView &v, int e, int episode) {
    if (!v.draw_m) return v.start_states[0];
    const uint32_t word = tabular_word(v, e, episode, 0, 0u);
    const uint32_t t = min(word, v.start_cum[v.M - 1] - 1u);
    int lo = 0, hi = v.M - 1;     // first m with start_cum[m] > t; start_cum[M - 1] > t
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (v.start_cum[mid] > t) hi = mid; else lo = mid + 1;
    }
    return v.start_states[lo];
}

__device__ __forceinline__ void tabular_begin_episode(const TabularView &v, int e, TabularEnv &s, float &reward, bool &terminal) {
    s.episode += 1;
    s.tick = 0;
    s.done = 0;
    s.ep_length = 0;
    s.ep_return = 0.0;
    s.state = tabular_draw_start(v, e, s.episode);
    reward = 0.0f;
    terminal = false;
}

// one env step; returns true when the episode finished.  An action outside the head is clamped into it: the tables are never read
// out of bounds (the protocol send checks the first batch of actions; the policy kernels only produce actions inside the head).
__device__ __forceinline__ bool tabular_step(const TabularView &v, int e, TabularEnv &s, int action, float &reward, bool &terminal,
                                             double &fin_return, int &fin_length, double &fin_score) {
    const int a = min(max(action, 0), v.A - 1);
    const size_t base = ((size_t)s.state * v.A + a) * v.K;
    int k = 0;
    if (v.draw_k) {
        const uint32_t word = tabular_word(v, e, s.episode, s.tick, 1u);
        const uint32_t *cum = v.cum + base;
        const uint32_t t = min(word, cum[v.K - 1] - 1u);
        for (int j = 0; j < v.K - 1; ++j) k += cum[j] <= t;
    }
    const int sn = v.next[base + k];
    const double r = v.reward[base + k];
    s.state = sn;
    s.tick += 1;
    s.ep_length += 1;
    s.ep_return += r;
    reward = (float)r;
    terminal = v.terminal[sn] != 0 || s.tick == v.horizon;
    s.done = terminal;
    if (terminal) {
        fin_return = s.ep_return;
        fin_length = s.ep_length;
        fin_score = v.score ? v.score[sn] : s.ep_return;
    }
    return terminal;
}

// values [16 chunk, 16 chunk + 16) of obs[state] -> row, 16-byte loads (table rows are obs_stride floats, 64-byte aligned), 8-byte
// stores (a row of the LDS observation tile is DP + 2 floats from the next)
__device__ __forceinline__ void tabular_copy_chunk(const TabularView &v, int state, int chunk, float *row) {
    const float4 *src = reinterpret_cast<const float4 *>(v.obs + (size_t)state * v.stride + 16 * chunk);
    float2 *dst = reinterpret_cast<float2 *>(row + 16 * chunk);
    float4 x[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] = src[q];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        dst[2 * q] = make_float2(x[q].x, x[q].y);
        dst[2 * q + 1] = make_float2(x[q].z, x[q].w);
    }
}

// The env adapter (env_adapters.hpp), in the shape of SynthRollEnv: the owner steps and leaves the new state index in Shared, the 16
// lanes of the env then copy its observation row, 16 values each.
struct TabularRollEnv {
    using View = TabularView;
    static View view(void *state, const pfa_tabular_config &c) { return tabular_view(state, c); }
    static constexpr bool kRefresh = true;
    struct Shared {
        int state[16];
    };
    TabularEnv s = {};
    int last_fin = 0;

    __device__ __forceinline__ void load(const View &v, int e, int, Shared &) { s = v.env[e]; }
    __device__ __forceinline__ void step(const View &v, int e, int le, Shared &sh, float *, int action, float &reward, bool &terminal) {
        last_fin = 0;
        if (s.done) {
            tabular_begin_episode(v, e, s, reward, terminal);
        } else {
            double fr, fs;
            int fl;
            if (tabular_step(v, e, s, action, reward, terminal, fr, fl, fs)) {
                episode_account(v.fin[e], fr, fl, fs);
                last_fin = 1;
            }
        }
        sh.state[le] = s.state;
    }
    __device__ __forceinline__ void refresh(const View &v, int, int le, int lo, Shared &sh, float *row) {
        if (16 * lo < v.stride) tabular_copy_chunk(v, sh.state[le], lo, row);
    }
    __device__ __forceinline__ void store(const View &v, int e, int, Shared &) {
        v.env[e] = s;
        v.fin[e].last_fin = last_fin;
    }
};

}  // namespace pfa
