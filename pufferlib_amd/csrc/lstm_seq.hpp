// lstm_seq.hpp — what the two forms of the recurrent training kernels share on the host side: the workgroup shape, the shape check and
// dispatch of csrc/lstm_seq.hip (exact fp32 MFMA products), and the entry point of csrc/lstm_seq_bf16.hip (the opt-in bf16x6 product
// form of the forward kernel) that pfa_lstm_seq_forward hands over to.
#pragma once
#include "common.hpp"
#include "lstm_tile.hpp"

namespace pfa {

constexpr int kSeqRT = 2;                 // row tiles per workgroup
constexpr int kSeqRows = 16 * kSeqRT;
constexpr int kBiasCols = kLG + kLH;      // per-workgroup partial column sums: dG (512) then dxe (128)

inline int check_seq_dims(const pfa_mlp_dims *d) {
    PFA_REQUIRE(d != nullptr, "lstm_seq: null dims");
    PFA_REQUIRE(d->hidden == kHidden, "lstm_seq: hidden must be %d (got %d)", kHidden, d->hidden);
    PFA_REQUIRE(d->obs_stride == 16 || d->obs_stride == 32 || d->obs_stride == 64 || d->obs_stride == 96 || d->obs_stride == 128 ||
                    d->obs_stride == 160,
                "lstm_seq: obs_stride must be one of 16/32/64/96/128/160 (got %d)", d->obs_stride);
    PFA_REQUIRE(d->num_actions >= 1 && d->num_actions <= 15, "lstm_seq: num_actions must be in 1..15 (got %d)", d->num_actions);
    return 0;
}

#define PFA_SEQ_DISPATCH_DP(dp, CALL)             \
    switch (dp) {                                 \
        case 16: { constexpr int DP = 16; CALL; } break;   \
        case 32: { constexpr int DP = 32; CALL; } break;   \
        case 64: { constexpr int DP = 64; CALL; } break;   \
        case 96: { constexpr int DP = 96; CALL; } break;   \
        case 160: { constexpr int DP = 160; CALL; } break; \
        default: { constexpr int DP = 128; CALL; } break;  \
    }

// csrc/lstm_seq_bf16.hip.  lstm_seq_bf16_bits: which directions take the bf16x6 kernels under the products switch as it stands now
// (bit 0 forward, bit 1 backward; 0 with the switch off) — what pfa_lstm_seq_path reports for every shape the kernels take.  The
// launcher reads its pack argument in the split form of pfa_lstm_pack_split.
int lstm_seq_bf16_bits();
int lstm_seq_fwd_bf16_launch(hipStream_t stream, const float *obs_tm, long long R, int Th, const float *params, const pfa_mlp_dims *dims,
                             const void *wsplit, float *xe, float *gates_act, float *Hs, float *Cs, int init_slot);

}  // namespace pfa
