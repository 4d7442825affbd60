// pixel_squared.hip — ocean Squared shown as uint8 frames: the state machine of squared_env.hpp (same state block, tape and
// statistics as squared.hip; the float grid the step writes is kept behind that block, N rows of v.stride floats) and a painter
// that turns each g x g grid into a frame of any (height, width, channels) in either channel order.
//
// One launch per send, two phases in a workgroup that owns `epw` consecutive envs (the last workgroup possibly fewer):
//   step    lane k < envs owned: squared_send_env on env k's grid row in the state
//   paint   everyone: the owned grids -> LDS as the two bytes a cell shows (even / odd channel), then the frames in 16-byte
//           chunks, consecutive lanes on consecutive chunks.  Which cell a byte shows does not depend on the env, so a chunk's 16
//           LDS offsets are worked out once (cell rows / columns of a pixel from two tables built per launch: no division per
//           byte; the (outer, middle, inner) position of a lane's next chunk by adding the digits of the stride) and every
//           owned env's 16 bytes are 16 byte reads + one 16-byte store.
// Roofline: height * width * channels bytes written per env and send (50 MB at 4096 x (64, 64, 3)), ~300 B of state touched:
// HBM-write bound; the LDS reads are one byte per byte written.
#include "common.hpp"
#include "squared_env.hpp"

#ifndef PFA_PIXEL_ENVS_PER_WG   // developer A/B builds: a fixed count instead of pixel_envs_per_wg()
#define PFA_PIXEL_ENVS_PER_WG 0
#endif

namespace pfa {

constexpr int kPixThreads = 256;
constexpr int kPixMaxEnvs = 8;                      // envs per workgroup, at most
constexpr int kPixMaxSide = 1024;                   // height, width: entries of the two tables
constexpr int kPixCells = 31 * 31 + 63;             // cells of the largest grid (d = 15), padded: odd-channel bytes follow at this offset
constexpr int kPixChunk = 16;
constexpr uint8_t kPixMarkEven = 255, kPixMarkOdd = 128;   // +1 (target marker); the agent (-1) shows the two swapped

struct PixView {
    float *grid;          // [N][v.stride] in the device state
    int height, width;
    int chunks;           // 16-byte chunks per frame
    int epw;              // envs per workgroup
    int st0, st1, st2;    // (outer, middle, inner) digits of the kPixThreads * 16 bytes between a lane's chunks
};

// The dims of a frame from the outside in: (height, width, C) channel-last, (C, height, width) channel-first.
template <int C, bool CL>
__device__ __forceinline__ void pix_dims(const PixView &p, int &d1, int &d2) {
    d1 = CL ? p.width : p.height;
    d2 = CL ? C : p.width;
}

// LDS offsets (into one env's cell bytes) of the 16 bytes that start at position (a0, a1, a2)
template <int C, bool CL>
__device__ __forceinline__ void pix_chunk_offsets(const PixView &p, const uint16_t *ytab, const uint16_t *xtab, int a0, int a1, int a2,
                                                  uint16_t (&off)[kPixChunk]) {
    if constexpr (CL) {
        int y = a0, x = a1, c = a2;
        int cell = ytab[y] + xtab[x];
#pragma unroll
        for (int k = 0; k < kPixChunk; ++k) {
            off[k] = (uint16_t)(cell + (c & 1) * kPixCells);
            if (++c == C) {
                c = 0;
                if (++x == p.width) {
                    x = 0;
                    ++y;           // == height only behind the frame's last byte: the tables have a spare entry
                }
                cell = ytab[y] + xtab[x];
            }
        }
    } else {
        int c = a0, y = a1, x = a2;
        int row = ytab[y] + (c & 1) * kPixCells;
#pragma unroll
        for (int k = 0; k < kPixChunk; ++k) {
            off[k] = (uint16_t)(row + xtab[x]);
            if (++x == p.width) {
                x = 0;
                if (++y == p.height) {
                    y = 0;
                    ++c;
                }
                row = ytab[y] + (c & 1) * kPixCells;
            }
        }
    }
}

// actions == nullptr: paint only (async_reset, after the seeding kernel of squared.hip wrote grid and live scalars)
template <int C, bool CL>
__global__ void __launch_bounds__(kPixThreads) pixel_squared_kernel(SquaredView v, PixView p, const long long *actions, uint8_t *obs,
                                                                    float *rewards, uint8_t *terminals, uint8_t *truncations,
                                                                    uint8_t *masks) {
    __shared__ uint8_t s_cell[kPixMaxEnvs][2 * kPixCells];      // [env][even-channel byte per cell | odd-channel byte per cell]
    __shared__ uint16_t s_ytab[kPixMaxSide + 1], s_xtab[kPixMaxSide + 1];   // pixel row -> first cell of its grid row; column -> grid column
    __shared__ uint16_t s_tc[kPixMaxEnvs][kMaxTargets];
    const int tid = threadIdx.x;
    const int e0 = blockIdx.x * p.epw;
    const int owned = v.n - e0 < p.epw ? v.n - e0 : p.epw;     // tail workgroup: fewer envs
    const int g = v.g, cells = g * g;

    if (actions != nullptr && tid < owned) {
        const int e = e0 + tid;
        squared_send_env(v, e, (int)actions[e], p.grid + (size_t)e * v.stride, s_tc[tid], rewards, terminals, truncations, masks);
    }
    for (int y = tid; y <= p.height; y += kPixThreads) s_ytab[y] = (uint16_t)(y < p.height ? (y * g / p.height) * g : 0);
    for (int x = tid; x <= p.width; x += kPixThreads) s_xtab[x] = (uint16_t)(x < p.width ? x * g / p.width : 0);
    __syncthreads();     // the owners' grid rows are visible to the workgroup

    for (int le = 0; le < owned; ++le) {
        const float *grid = p.grid + (size_t)(e0 + le) * v.stride;
        for (int i = tid; i < cells; i += kPixThreads) {
            const float f = grid[i];
            s_cell[le][i] = f > 0.0f ? kPixMarkEven : (f < 0.0f ? kPixMarkOdd : 0);
            s_cell[le][kPixCells + i] = f > 0.0f ? kPixMarkOdd : (f < 0.0f ? kPixMarkEven : 0);
        }
    }
    __syncthreads();

    int d1, d2;
    pix_dims<C, CL>(p, d1, d2);
    int a2 = (tid * kPixChunk) % d2, t = (tid * kPixChunk) / d2;   // this lane's first chunk: the only divisions of the paint phase
    int a1 = t % d1, a0 = t / d1;
    const size_t frame_bytes = (size_t)p.chunks * kPixChunk;
    uint8_t *out = obs + (size_t)e0 * frame_bytes;
    for (int q = tid; q < p.chunks; q += kPixThreads) {
        uint16_t off[kPixChunk];
        pix_chunk_offsets<C, CL>(p, s_ytab, s_xtab, a0, a1, a2, off);
        for (int le = 0; le < owned; ++le) {
            const uint8_t *cell = s_cell[le];
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                w[k] = (uint32_t)cell[off[4 * k]] | ((uint32_t)cell[off[4 * k + 1]] << 8) | ((uint32_t)cell[off[4 * k + 2]] << 16) |
                       ((uint32_t)cell[off[4 * k + 3]] << 24);
            *reinterpret_cast<uint4 *>(out + (size_t)le * frame_bytes + (size_t)q * kPixChunk) = make_uint4(w[0], w[1], w[2], w[3]);
        }
        a2 += p.st2;     // digits of the next chunk: each sum stays below twice its dim, one carry each
        if (a2 >= d2) { a2 -= d2; a1 += 1; }
        a1 += p.st1;
        if (a1 >= d1) { a1 -= d1; a0 += 1; }
        a0 += p.st0;
    }
}

// Envs per workgroup.  What a workgroup does before it paints (the tables, two barriers, the grids into LDS, a lane's first position)
// costs the same for one env as for eight, so it owns as many as still leave every CU four workgroups: at 4096 x (64, 64, 3) a send
// takes 29.5 us with one env per workgroup, 21.1 with two, 17.5 with four (1024 workgroups) and 17.6 with eight.
static int pixel_envs_per_wg(int num_envs) {
    if (PFA_PIXEL_ENVS_PER_WG > 0) return PFA_PIXEL_ENVS_PER_WG < kPixMaxEnvs ? PFA_PIXEL_ENVS_PER_WG : kPixMaxEnvs;
    int epw = 1;
    while (epw < kPixMaxEnvs && num_envs / (2 * epw) >= 1024) epw *= 2;
    return epw;
}

static bool pixel_channel_last(const pfa_pixel_config *p) { return p->sc == 1 && p->sx == p->channels && p->sy == p->width * p->channels; }
static bool pixel_channel_first(const pfa_pixel_config *p) { return p->sx == 1 && p->sy == p->width && p->sc == p->height * p->width; }

static int check_pixel(const pfa_squared_config *c, const pfa_pixel_config *p) {
    PFA_REQUIRE(c != nullptr && p != nullptr, "pixel_squared: null config");
    if (pfa_squared_state_bytes(c) == 0) return -2;     // squared.hip's own checks of its config, its message kept
    const int g = 2 * c->distance_to_target + 1;
    PFA_REQUIRE(c->obs_stride == (g * g + 15) / 16 * 16, "pixel_squared: the state grid has rows of round_up(g*g, 16) = %d floats, got obs_stride %d",
                (g * g + 15) / 16 * 16, c->obs_stride);
    PFA_REQUIRE(p->height >= g && p->width >= g && p->height <= kPixMaxSide && p->width <= kPixMaxSide,
                "pixel_squared: height and width must be in %d..%d (one pixel per grid cell at least), got %d x %d", g, kPixMaxSide, p->height, p->width);
    PFA_REQUIRE(p->channels >= 1 && p->channels <= 4, "pixel_squared: channels must be in 1..4, got %d", p->channels);
    PFA_REQUIRE((p->height * p->width * p->channels) % kPixChunk == 0, "pixel_squared: frames are written in 16-byte chunks, %d x %d x %d bytes is no multiple",
                p->height, p->width, p->channels);
    PFA_REQUIRE(pixel_channel_last(p) || pixel_channel_first(p),
                "pixel_squared: byte strides (sc, sy, sx) = (%d, %d, %d) are neither a dense (H, W, C) nor a dense (C, H, W) frame", p->sc, p->sy, p->sx);
    return 0;
}

template <int C, bool CL>
static void pixel_launch_as(const SquaredView &v, const PixView &p, const int64_t *actions, uint8_t *obs, float *rewards, uint8_t *terminals,
                            uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    const unsigned blocks = (unsigned)((v.n + p.epw - 1) / p.epw);
    hipLaunchKernelGGL((pixel_squared_kernel<C, CL>), dim3(blocks), dim3(kPixThreads), 0, (hipStream_t)stream, v, p, (const long long *)actions, obs,
                       rewards, terminals, truncations, masks);
}

static int pixel_launch(void *state, const pfa_squared_config *cfg, const pfa_pixel_config *pix, const int64_t *actions, uint8_t *obs, float *rewards,
                        uint8_t *terminals, uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    const SquaredView v = squared_view(state, *cfg);
    const bool cl = pixel_channel_last(pix);     // (one channel: both orders are the same bytes)
    PixView p;
    p.grid = (float *)((char *)state + pfa_squared_state_bytes(cfg));
    p.height = pix->height;
    p.width = pix->width;
    p.chunks = pix->height * pix->width * pix->channels / kPixChunk;
    p.epw = pixel_envs_per_wg(cfg->num_envs);
    const int d1 = cl ? pix->width : pix->height, d2 = cl ? pix->channels : pix->width, step = kPixThreads * kPixChunk;
    p.st2 = step % d2;
    p.st1 = step / d2 % d1;
    p.st0 = step / d2 / d1;
#define PFA_PIXEL_CASE(C)                                                                                             \
    case C:                                                                                                           \
        if (cl) pixel_launch_as<C, true>(v, p, actions, obs, rewards, terminals, truncations, masks, stream);         \
        else pixel_launch_as<C, false>(v, p, actions, obs, rewards, terminals, truncations, masks, stream);           \
        break;
    switch (pix->channels) {
        PFA_PIXEL_CASE(1)
        PFA_PIXEL_CASE(2)
        PFA_PIXEL_CASE(3)
        PFA_PIXEL_CASE(4)
    }
#undef PFA_PIXEL_CASE
    PFA_LAUNCH_CHECK();
    return 0;
}

}  // namespace pfa

using namespace pfa;

extern "C" size_t pfa_pixel_squared_state_bytes(const pfa_squared_config *cfg, const pfa_pixel_config *pix) {
    if (check_pixel(cfg, pix)) return 0;
    return pfa_squared_state_bytes(cfg) + (size_t)cfg->num_envs * cfg->obs_stride * sizeof(float);
}

extern "C" int pfa_pixel_squared_async_reset(void *state, const pfa_squared_config *cfg, const pfa_pixel_config *pix, int64_t seed, uint8_t *obs,
                                             float *rewards, uint8_t *terminals, uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    if (int rc = check_pixel(cfg, pix)) return rc;
    PFA_REQUIRE(state && obs && rewards && terminals && truncations && masks, "pixel_squared.async_reset: null buffer");
    float *grid = (float *)((char *)state + pfa_squared_state_bytes(cfg));
    if (int rc = pfa_squared_async_reset(state, cfg, seed, grid, rewards, terminals, truncations, masks, stream)) return rc;
    return pixel_launch(state, cfg, pix, nullptr, obs, rewards, terminals, truncations, masks, stream);
}

extern "C" int pfa_pixel_squared_send(void *state, const pfa_squared_config *cfg, const pfa_pixel_config *pix, const int64_t *actions, uint8_t *obs,
                                      float *rewards, uint8_t *terminals, uint8_t *truncations, uint8_t *masks, pfa_stream_t stream) {
    if (int rc = check_pixel(cfg, pix)) return rc;
    PFA_REQUIRE(state && actions && obs && rewards && terminals && truncations && masks, "pixel_squared.send: null buffer");
    return pixel_launch(state, cfg, pix, actions, obs, rewards, terminals, truncations, masks, stream);
}
