// catch_row_env.hpp — Catch (catch_env.hpp: catch_send, the same Philox counter and 'PC' key as PixelCatch) as flat float32 rows: the
// env adapter (env_adapters.hpp) the protocol send kernel and the fused MLP / recurrent rollout skeletons run.  The state is
// PixelCatch's (CatchEnv + EpisodeFin per env; only history slot 0 is shown), so equal (rows, cols, seed, env_offset) and equal actions
// walk the same episodes in both families.
//
// Observation rows of `stride` floats, zero behind the real values:
//   grid     rows * cols values: 1 at the ball's cell r * cols + c and at the paddle's cell (rows - 1) * cols + p, 0 elsewhere.  The
//            ball's horizontal velocity is not shown: it follows from two consecutive rows (the memory form)
//   coords   (r / (rows - 1), c / (cols - 1), p / (cols - 1)) and, with `velocities`, vx in {-1, 0, 1}: each quotient one IEEE f32
//            division of two small integers; rows of 16 floats
//
// The row is computed, never copied: there is no table and no load on the per-step chain.  The owner lane steps (catch_send) and
// holds (r, c, p, vx) in registers; behind the skeleton's barrier its word r | c << 8 | p << 16 | (vx + 1) << 24 goes round the env's
// 16 lanes as a DPP row maximum over (word, 0, ..., 0) — four v_max_i32_dpp, no LDS round trip — and lane `lo` then forms float `lo`
// of EVERY 16-float chunk of the row: two integer compares per value for `grid` (chunk offset against ball - lo and paddle - lo),
// one division and a select over four values for `coords`.  That is another split of the row than the adapters that copy
// (SynthRollEnv, TabularRollEnv: lane lo owns chunk lo): every lane of the env works whatever the row's width, and a lane's stores
// are one bank apart from its neighbours'.
#pragma once
#include "catch_env.hpp"
#include "lane_ops.hpp"

namespace pfa {

constexpr int kCatchRowMaxCells = 160;   // grid form: the widest row of the recurrent tier
constexpr int kCatchRowMaxSide = 256;    // a row and two columns travel in a byte each of the env's word

struct CatchRowView : CatchView {
    int stride;        // floats per observation row
    int paddle0;       // (rows - 1) * cols: cell of the paddle row's first column
    bool coords, velocities;
};

__device__ __forceinline__ int catch_row_word(const CatchEnv &s) {
    return (int)s.r[0] | ((int)s.c[0] << 8) | ((int)s.p[0] << 16) | ((s.vx + 1) << 24);
}

// Floats lo, 16 + lo, 32 + lo, ... of the env's observation row from the env's word.
__device__ __forceinline__ void catch_row_write(const CatchRowView &v, int word, int lo, float *row) {
    const int r = word & 0xff, c = (word >> 8) & 0xff, p = (word >> 16) & 0xff;
    if (v.coords) {
        const int num = lo == 0 ? r : (lo == 1 ? c : p), den = lo == 0 ? v.rows - 1 : v.cols - 1;   // den >= 1 (check)
        const float quotient = (float)num / (float)den;
        const float vx = v.velocities ? (float)((word >> 24) - 1) : 0.0f;
        row[lo] = lo < 3 ? quotient : (lo == 3 ? vx : 0.0f);
    } else {
        const int ball = r * v.cols + c - lo, paddle = v.paddle0 + p - lo;    // the chunk offset at which this lane's float is 1
        for (int j = 0; j < v.stride; j += 16) row[j + lo] = (j == ball || j == paddle) ? 1.0f : 0.0f;
    }
}

int check_catch_config(const pfa_catch_config *c);   // catch.hip

// kLanes: the 16 lanes of a DPP row are the env's (the fused rollouts).  false: one thread is the env's owner and all 16 of its
// lanes in turn (env_send_kernel, the reset kernel), so there is nobody to hand the word to.
template <bool kLanes>
struct CatchRowEnvT {
    using View = CatchRowView;
    using Config = pfa_catch_config;
    static constexpr const char *kName = "catch";
    static constexpr bool kRefresh = true;
    struct Shared {};
    CatchEnv s = {};
    int last_fin = 0;

    static int check(const Config *c) { return check_catch_config(c); }
    static size_t state_bytes(int n) { return (size_t)n * (sizeof(CatchEnv) + sizeof(EpisodeFin)); }
    static int stride(const Config &c) { return c.obs_stride; }
    static View view(void *state, const Config &c) {
        View v;
        v.env = (CatchEnv *)state;
        v.fin = (EpisodeFin *)((char *)state + (size_t)c.num_envs * sizeof(CatchEnv));
        v.n = c.num_envs;
        v.rows = c.rows;
        v.cols = c.cols;
        v.key0 = (uint32_t)c.seed;
        v.key1 = 0x5043u ^ (uint32_t)(c.seed >> 32);   // 'PC': PixelCatch's key, the twin walks the same episodes
        v.env_offset = c.env_offset;
        v.stride = c.obs_stride;
        v.paddle0 = (c.rows - 1) * c.cols;
        v.coords = c.obs_form == PFA_CATCH_OBS_COORDS;
        v.velocities = c.velocities != 0;
        return v;
    }

    __device__ __forceinline__ void load(const View &v, int e, int, Shared &) { s = v.env[e]; }
    __device__ __forceinline__ void reset(const View &v, int e) {
        s = CatchEnv{};
        s.episode = -1;
        catch_begin_episode(v, e, s);
        v.fin[e] = EpisodeFin{};
        last_fin = 0;
    }
    __device__ __forceinline__ void step(const View &v, int e, int, Shared &, float *, int action, float &reward, bool &terminal) {
        last_fin = catch_send(v, e, s, action, reward, terminal) ? 1 : 0;
    }
    // every lane of the env (a lane that is not the owner holds no state: its word is 0, below every owner's)
    __device__ __forceinline__ void refresh(const View &v, int, int, int lo, Shared &, float *row) {
        int word = (!kLanes || lo == 0) ? catch_row_word(s) : 0;
        if constexpr (kLanes) word = row16_max_i32(word);
        catch_row_write(v, word, lo, row);
    }
    __device__ __forceinline__ void store(const View &v, int e, int, Shared &) {
        v.env[e] = s;
        v.fin[e].last_fin = last_fin;
    }
};
using CatchRowEnv = CatchRowEnvT<true>;
using CatchRowSendEnv = CatchRowEnvT<false>;

}  // namespace pfa
