// env_adapters.hpp — one definition of "what one send() does to one env" per device env family, shared by the family's protocol send
// kernel (env_send_kernel below), the fused recurrent rollout (rollout_lstm_kernel, lstm_fused.hip) and, for the families that have
// one, the fused MLP rollout (rollout_mlp_env_kernel, rollout_env.hpp; Squared keeps its tuned kernel in rollout.hip).
//
// An env adapter is a plain struct that holds the env's state in registers of its owner thread (in the fused rollouts: lane 0 of the
// env's 16-lane sampling group) and supplies what differs per env family:
//   View / view()   the device view of the vecenv state and how the entry point's config maps to it
//   Shared          what the env keeps next to its observation rows for the other lanes of the env (empty: costs nothing); LDS in the
//                   fused rollouts, a per-thread local with le = 0 in env_send_kernel
//   load / store    owner thread: state in before the first step / out after the last one; store leaves "finished by the last step"
//                   in EpisodeFin::last_fin (what recv() hands out as infos)
//   step            owner thread, after the scalars of row (e, t) are stored: reset from the tape (flagging a tape underrun) or apply the
//                   sampled action, with the EpisodeStats bookkeeping; writes `reward` / `terminal` of the next row and the env's
//                   observation row (`row`: the env's row of the LDS tile, or of the live buffer)
//   refresh         all 16 lanes of the env, after the barrier that follows step, only where kRefresh (a second barrier
//                   follows it): lane `lo` rewrites values [16 lo, 16 lo + 16) of the row from what step left in Shared
#pragma once
#include "common.hpp"
#include "squared_env.hpp"
#include "memory_env.hpp"
#include "synth_env.hpp"

namespace pfa {

struct SquaredRollEnv {
    using View = SquaredView;
    static View view(void *state, const pfa_squared_config &c) { return squared_view(state, c); }
    static constexpr bool kRefresh = false;
    struct Shared {
        uint16_t tg[16 * kMaxTargets];   // target cells per env
    };
    SquaredEnv s;

    __device__ __forceinline__ void load(const View &v, int e, int le, Shared &sh) {
        squared_load(v, e, s);
        for (int t = 0; t < v.nt; ++t) sh.tg[le * kMaxTargets + t] = v.tgt[(size_t)t * v.n + e];
    }
    __device__ __forceinline__ void step(const View &v, int e, int le, Shared &sh, float *grid, int action, float &reward,
                                         bool &terminal) {
        uint16_t *tc = sh.tg + le * kMaxTargets;
        if (s.done) {
            if ((long long)s.rounds >= v.hdr->rounds_filled) v.hdr->underrun = 1;
            const uint16_t *tr = v.tape + (size_t)(s.rounds % (uint32_t)v.tape_rounds) * v.nt * v.n;
            squared_reset(v, e, s, grid, tr, tc, reward, terminal);
            s.rounds += 1;
        } else {
            bool fin;
            double fr, fs;
            int fl;
            squared_step(v, s, grid, tc, action, reward, terminal, fin, fr, fl, fs);
        }
    }
    __device__ __forceinline__ void refresh(const View &, int, int, int, Shared &, float *) {}
    __device__ __forceinline__ void store(const View &v, int e, int le, Shared &sh) {
        squared_store(v, e, s);
        for (int t = 0; t < v.nt; ++t) v.tgt[(size_t)t * v.n + e] = sh.tg[le * kMaxTargets + t];
        v.fin[e] = 0;
    }
};

// ocean Memory (memory_env.hpp; observation rows of 16 floats, one real column): the env that NEEDS the recurrent state.
struct MemoryRollEnv {
    using View = MemoryView;
    static View view(void *state, const pfa_memory_config &c) { return memory_view(state, c); }
    static constexpr bool kRefresh = false;
    struct Shared {};
    MemoryEnv s = {};
    int last_fin = 0;

    __device__ __forceinline__ void load(const View &v, int e, int, Shared &) { s = v.env[e]; }
    __device__ __forceinline__ void step(const View &v, int e, int, Shared &, float *row, int action, float &reward, bool &terminal) {
        float o;
        last_fin = 0;
        if (s.done) {   // auto-reset row (vector.py:144-151): the action is ignored, the next solution comes off the tape
            if (s.rounds >= v.hdr->rounds_filled) v.hdr->underrun = 1;
            const uint32_t bits = v.tape[(size_t)(s.rounds % v.tape_rounds) * v.n + e];
            const long long rounds = s.rounds + 1;
            memory_begin_episode(s, bits, o, reward, terminal);
            s.rounds = rounds;
        } else {
            double fr, fs;
            int fl;
            if (memory_step(v, s, action, o, reward, terminal, fr, fl, fs)) {
                episode_account(v.fin[e], fr, fl, fs);
                last_fin = 1;
            }
        }
        row[0] = o;
    }
    __device__ __forceinline__ void refresh(const View &, int, int, int, Shared &, float *) {}
    __device__ __forceinline__ void store(const View &v, int e, int, Shared &) {
        v.env[e] = s;
        v.fin[e].last_fin = last_fin;
    }
};

// The synthetic byte-row env of BASELINE configs[2] (synth_env.hpp; rows of DP = obs_stride floats).  The 16 lanes of an env's
// sampling group regenerate its observation row after the step, 16 values per lane (one Philox call each).
struct SynthRollEnv {
    using View = SynthView;
    static View view(void *state, const pfa_synth_config &c) { return synth_view(state, c); }
    static constexpr bool kRefresh = true;
    struct Shared {
        int tick[16], episode[16];   // the owner's (tick, episode) after the step, for the other lanes of the env
    };
    SynthEnv s = {};
    int last_fin = 0;

    __device__ __forceinline__ void load(const View &v, int e, int, Shared &) { s = v.env[e]; }
    __device__ __forceinline__ void step(const View &v, int e, int le, Shared &sh, float *row, int action, float &reward, bool &terminal) {
        last_fin = 0;
        if (s.done) {
            synth_begin_episode(s, reward, terminal);
        } else {
            double fr, fs;
            int fl;
            if (synth_step(v, s, action, (int)row[0], reward, terminal, fr, fl, fs)) {
                episode_account(v.fin[e], fr, fl, fs);
                last_fin = 1;
            }
        }
        sh.tick[le] = s.tick;
        sh.episode[le] = s.episode;
    }
    __device__ __forceinline__ void refresh(const View &v, int e, int le, int lo, Shared &sh, float *row) {
        if (lo * 16 < v.values) {   // the next observation row of this env, 16 values per lane
            float vals[16];
            synth_chunk(v, e, sh.episode[le], sh.tick[le], lo, vals);
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (lo * 16 + k < v.values) row[lo * 16 + k] = vals[k];
        }
    }
    __device__ __forceinline__ void store(const View &v, int e, int, Shared &) {
        v.env[e] = s;
        v.fin[e].last_fin = last_fin;
    }
};

// Owner thread of the fused rollouts, after store: what the next recv() returns for env e beside its observation row.  (`terminal`
// arrives as the byte to store: as a bool it comes back from the inliner as a compare the kernels did not have.  The experience-row
// store has no such helper: every spelling of it moved an s_nop of the Tabular MLP instantiations — docs/lab-notebook.md.)
__device__ __forceinline__ void store_live(int e, float reward, uint8_t terminal, float *live_rew, uint8_t *live_term,
                                           uint8_t *live_trunc, uint8_t *live_mask) {
    live_rew[e] = reward;
    live_term[e] = terminal;
    live_trunc[e] = 0;
    live_mask[e] = 1;
}

// The protocol send() of a family over its adapter, one thread per env: the thread is the owner and all 16 lanes of its env, `row` is
// the env's row of the live observation buffer (`stride` floats apart).
template <class Env>
__global__ void __launch_bounds__(256) env_send_kernel(typename Env::View v, int stride, const long long *actions, float *obs, float *rewards,
                                                      uint8_t *terminals, uint8_t *truncations, uint8_t *masks) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= v.n) return;
    Env env;
    typename Env::Shared sh;
    float *row = obs + (size_t)e * stride;
    float reward;
    bool terminal;
    env.load(v, e, 0, sh);
    env.step(v, e, 0, sh, row, (int)actions[e], reward, terminal);
    if constexpr (Env::kRefresh) {
        for (int lo = 0; lo < 16; ++lo) env.refresh(v, e, 0, lo, sh, row);
    }
    env.store(v, e, 0, sh);
    rewards[e] = reward;
    terminals[e] = terminal ? 1 : 0;
    truncations[e] = 0;
    masks[e] = 1;
}

// Host side of a family's `*_send` entry point, which has checked its own config: `name` prefixes the error text.
template <class Env>
static int launch_env_send(const char *name, void *state, const typename Env::View &v, int stride, const int64_t *actions, float *obs,
                           float *rewards, uint8_t *terminals, uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    PFA_REQUIRE(state && actions && obs && rewards && terminals && truncations && masks, "%s: null buffer", name);
    hipLaunchKernelGGL(env_send_kernel<Env>, dim3((unsigned)((v.n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, v, stride,
                       (const long long *)actions, obs, rewards, terminals, truncations, masks);
    PFA_LAUNCH_CHECK();
    return 0;
}

}  // namespace pfa
