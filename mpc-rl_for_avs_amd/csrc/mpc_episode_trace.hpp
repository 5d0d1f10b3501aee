// mpc_episode_trace.hpp - the step-by-step record of the episodes of a closed-loop evaluation that someone will look at, next
// to mpc_episode_stats.hpp: every environment keeps the last W steps of its current episode in rings, and an episode that ends
// and is selected (by its outcome) is copied, in chronological order, to the next free slot of a store with capacity C.  The
// functions below are shared by the two kernels of mpc_episode_trace in mpc_engine.hip (claim: who gets which slot; frame:
// the append and the copy) and their host build (tests/cpu_episode_trace_harness.cpp).
//
// The model.  An episode of environment b with T steps has scenes s_0 .. s_T (observations [R][8] f32; s_T is the scene after
// the last step, before the auto-reset) and one frame per step t: the action [2] f64 as commanded, the reward f32, the solve's
// status and iteration count, flags (bit 0 done, 1 truncated, 2 crashed, 3 arrived) and, with a perception model, what the
// agent acted on (seen [R][8] f32).  Its outcome is a bit set: 1 collision (crashed on any step), 2 truncated, 4 success
// (arrived), 8 unsolved (a solve that is not MPC_STATUS_IS_SOLVED) - the facts mpc_episode_stats records.  It is selected when
// its ordinal j < Q (the episodes the accounting records) and keep & 16 (all) or outcome & keep & 15.  Selected episodes take
// slots 0, 1, .. in the order (launch on which they ended, environment index); one that finds the store full is counted as
// dropped.  A kept episode holds its last L = min(T, W) steps, first = T - L: kept frame i is step first + i (i < L), kept
// scene i is s_{first + i} (i <= L).  Entries past L are not written.
//
// Running state of environment b (planar): state_i32 [4][B] = steps of the current episode, crashed so far, unsolved so far,
// the ordinal j (saturates at Q: such an environment writes nothing at all).
// Rings of environment b: ring_scene [B][W + 1][R][8] f32 (scene t at index t mod (W + 1)); ring_seen [B][W][R][8] f32 or
// NULL, ring_act [B][W][2] f64, ring_reward [B][W] f32, ring_i32 [B][W][3] = status, iters, flags (frame t at index t mod W).
// Work array: slot [B] i32, written by the claim for the frame kernel: the slot of an episode that ends now, else -1.
// Store: kept_scene [C][W + 1][R][8], kept_seen [C][W][R][8] or NULL, kept_act [C][W][2], kept_reward [C][W], kept_i32
// [C][W][3]; index [C][6] i32 = b, j, T, first, outcome, the launch the episode ended on (1-based since the reset launch);
// counts [4] i64 = matched, kept, dropped, launches (matched = kept + dropped).
//
// Every copy is a lane-strided loop (lane, lanes): the kernel passes its thread index and workgroup size, the host build
// (0, 1).  A scene is 2 R chunks of 16 bytes.  Every ring and store index is reduced to its range before use (unsigned
// remainder, slot checked against C), so no content of the running state can make an access leave its buffer.
#pragma once

#include <stdint.h>
#include <string.h>

#include "mpc_core.hpp"

namespace mpc {
namespace trace {

enum { kSteps = 0, kCrashed = 1, kUnsolved = 2, kOrdinal = 3, kStateI32 = 4 };
enum { kIdxEnv = 0, kIdxOrdinal = 1, kIdxSteps = 2, kIdxFirst = 3, kIdxOutcome = 4, kIdxLaunch = 5, kIndex = 6 };
enum { kMatched = 0, kKept = 1, kDropped = 2, kLaunches = 3, kCounts = 4 };
enum { kFrameStatus = 0, kFrameIters = 1, kFrameFlags = 2, kFrameI32 = 3 };
enum { kCollision = 1, kTruncated = 2, kSuccess = 4, kUnsolvedBit = 8, kKeepAll = 16 };
enum { kFlagDone = 1, kFlagTruncated = 2, kFlagCrashed = 4, kFlagArrived = 8 };
constexpr int kCols = 8, kMaxRows = 17, kMaxWindow = 4096;   // observation columns, MPC_MAX_OTHERS + 1, the largest W

struct StepInputs {              // one policy step of B environments
    const float *terminal_obs;   // [B][R][8] the scene after the step, before the auto-reset
    const float *obs;            // [B][R][8] what the next step starts from
    const float *seen;           // [B][R][8] what the agent acted on, or NULL
    const double *action;        // [B][2]
    const float *reward;         // [B]
    const uint8_t *done, *truncated, *crashed, *arrived;   // [B]
    const int32_t *status, *iters;                         // [B]
};

struct Recorder {
    int B, R, Q, W, C, keep;
    int32_t *state_i32;          // [4][B]
    float *ring_scene, *ring_seen;
    double *ring_act;
    float *ring_reward;
    int32_t *ring_i32, *slot;
    float *kept_scene, *kept_seen;
    double *kept_act;
    float *kept_reward;
    int32_t *kept_i32, *index;
    int64_t *counts;
};

MPC_HD bool solved(int32_t st) { return st == 0 || (st >= 5 && st <= 7); }   // MPC_STATUS_IS_SOLVED

MPC_HD int32_t outcome(bool crashed_ever, bool truncated, bool arrived, bool unsolved_ever) {
    return (crashed_ever ? kCollision : 0) | (truncated ? kTruncated : 0) | (arrived ? kSuccess : 0) |
           (unsolved_ever ? kUnsolvedBit : 0);
}

MPC_HD bool selected(int32_t keep, int32_t oc) { return (keep & kKeepAll) != 0 || (oc & keep & 15) != 0; }

// the outcome of environment b's episode if it ended on this step: the running state as it is BEFORE the step, and the step
MPC_HD int32_t outcome_now(const Recorder &r, const StepInputs &in, int b) {
    const size_t B = (size_t)r.B;
    const int32_t *si = r.state_i32 + b;
    return outcome(si[kCrashed * B] != 0 || in.crashed[b] != 0, in.truncated[b] != 0, in.arrived[b] != 0,
                   si[kUnsolved * B] != 0 || !solved(in.status[b]));
}

// the claim's question: does environment b end an episode on this step that is to be kept?
MPC_HD bool ends_selected(const Recorder &r, const StepInputs &in, int b) {
    return r.state_i32[kOrdinal * (size_t)r.B + b] < r.Q && in.done[b] != 0 && selected(r.keep, outcome_now(r, in, b));
}

MPC_HD int32_t frame_flags(const StepInputs &in, int b) {
    return (in.done[b] ? kFlagDone : 0) | (in.truncated[b] ? kFlagTruncated : 0) | (in.crashed[b] ? kFlagCrashed : 0) |
           (in.arrived[b] ? kFlagArrived : 0);
}

// the claim's bookkeeping after `m` environments were matched on this launch, `kept_before` slots being taken: slot of the
// episode of rank `rank` among them (or -1), and the counts
MPC_HD int32_t slot_of(int64_t kept_before, int64_t rank, int C) {
    const int64_t s = kept_before + rank;
    return s < (int64_t)C ? (int32_t)s : -1;
}

MPC_HD void advance_counts(int64_t *counts, int64_t m, int C) {
    const int64_t room = (int64_t)C - counts[kKept];
    const int64_t k = m < room ? m : (room > 0 ? room : 0);
    counts[kMatched] += m;
    counts[kKept] += k;
    counts[kDropped] += m - k;
    counts[kLaunches] += 1;
}

MPC_HD void copy16(float *dst, const float *src) {           // one aligned 16-byte chunk
#if defined(__HIP_DEVICE_COMPILE__)
    *reinterpret_cast<float4 *>(dst) = *reinterpret_cast<const float4 *>(src);
#else
    memcpy(dst, src, 16);
#endif
}

MPC_HD void copy_scene(float *dst, const float *src, int R, int lane, int lanes) {
    for (int e = lane; e < 2 * R; e += lanes) copy16(dst + 4 * e, src + 4 * e);
}

MPC_HD unsigned wrap(int32_t t, int n) { return (unsigned)t % (unsigned)n; }

// frame t of environment b from the step's inputs, and the scene the step led to (s_{t + 1})
MPC_HD void append(const Recorder &r, const StepInputs &in, int b, int32_t t, int lane, int lanes) {
    const size_t W = (size_t)r.W, scene = (size_t)r.R * kCols;
    const size_t f = (size_t)b * W + wrap(t, r.W);
    copy_scene(r.ring_scene + ((size_t)b * (W + 1) + wrap(t + 1, r.W + 1)) * scene, in.terminal_obs + (size_t)b * scene, r.R,
               lane, lanes);
    if (r.ring_seen) copy_scene(r.ring_seen + f * scene, in.seen + (size_t)b * scene, r.R, lane, lanes);
    if (lane == 0) {
        r.ring_act[f * 2] = in.action[(size_t)b * 2];
        r.ring_act[f * 2 + 1] = in.action[(size_t)b * 2 + 1];
        r.ring_reward[f] = in.reward[b];
        r.ring_i32[f * kFrameI32 + kFrameStatus] = in.status[b];
        r.ring_i32[f * kFrameI32 + kFrameIters] = in.iters[b];
        r.ring_i32[f * kFrameI32 + kFrameFlags] = frame_flags(in, b);
    }
}

// `count` ring entries of `unit` elements from entry `start` on, in ring order, to dst: two contiguous pieces
template <class T>
MPC_HD void copy_ring(T *dst, const T *ring, size_t unit, unsigned start, unsigned count, unsigned modulus, int lane, int lanes) {
    const unsigned head = count < modulus - start ? count : modulus - start;
    const size_t n0 = (size_t)head * unit, n1 = (size_t)(count - head) * unit;
    const T *src = ring + (size_t)start * unit;
    for (size_t e = lane; e < n0; e += lanes) dst[e] = src[e];
    for (size_t e = lane; e < n1; e += lanes) dst[n0 + e] = ring[e];
}

MPC_HD void copy_ring16(float *dst, const float *ring, size_t chunks, unsigned start, unsigned count, unsigned modulus, int lane,
                        int lanes) {
    const unsigned head = count < modulus - start ? count : modulus - start;
    const size_t n0 = (size_t)head * chunks, n1 = (size_t)(count - head) * chunks;
    const float *src = ring + (size_t)start * chunks * 4;
    for (size_t e = lane; e < n0; e += lanes) copy16(dst + 4 * e, src + 4 * e);
    for (size_t e = lane; e < n1; e += lanes) copy16(dst + 4 * (n0 + e), ring + 4 * e);
}

// the episode of environment b that ended after T steps (its frames and scenes are all in the rings) to slot s of the store,
// chronologically; lane 0 writes the index row.  The caller has checked 0 <= s < C.
MPC_HD void commit(const Recorder &r, int b, int32_t s, int32_t T, int32_t j, int32_t oc, int lane, int lanes) {
    const size_t W = (size_t)r.W, scene = (size_t)r.R * kCols, chunks = (size_t)2 * r.R;
    const int32_t L = T < r.W ? T : r.W, first = T - L;
    const unsigned f0 = wrap(first, r.W), s0 = wrap(first, r.W + 1);
    copy_ring16(r.kept_scene + (size_t)s * (W + 1) * scene, r.ring_scene + (size_t)b * (W + 1) * scene, chunks, s0,
                (unsigned)L + 1, (unsigned)r.W + 1, lane, lanes);
    if (r.ring_seen)
        copy_ring16(r.kept_seen + (size_t)s * W * scene, r.ring_seen + (size_t)b * W * scene, chunks, f0, (unsigned)L,
                    (unsigned)r.W, lane, lanes);
    copy_ring(r.kept_act + (size_t)s * W * 2, r.ring_act + (size_t)b * W * 2, 2, f0, (unsigned)L, (unsigned)r.W, lane, lanes);
    copy_ring(r.kept_reward + (size_t)s * W, r.ring_reward + (size_t)b * W, 1, f0, (unsigned)L, (unsigned)r.W, lane, lanes);
    copy_ring(r.kept_i32 + (size_t)s * W * kFrameI32, r.ring_i32 + (size_t)b * W * kFrameI32, kFrameI32, f0, (unsigned)L,
              (unsigned)r.W, lane, lanes);
    if (lane == 0) {
        int32_t *ix = r.index + (size_t)s * kIndex;
        ix[kIdxEnv] = b;
        ix[kIdxOrdinal] = j;
        ix[kIdxSteps] = T;
        ix[kIdxFirst] = first;
        ix[kIdxOutcome] = oc;
        ix[kIdxLaunch] = (int32_t)r.counts[kLaunches];
    }
}

// s_0 of environment b's next episode
MPC_HD void begin_episode(const Recorder &r, const float *obs, int b, int lane, int lanes) {
    const size_t scene = (size_t)r.R * kCols;
    copy_scene(r.ring_scene + (size_t)b * ((size_t)r.W + 1) * scene, obs + (size_t)b * scene, r.R, lane, lanes);
}

// What one launch does for environment b, in four parts.  `at(k)` is called between them: the kernel passes a workgroup
// barrier (part k + 1 reads what other lanes wrote in part k, or overwrites what they read), the host build nothing.
//   0  read the running state and the step (every lane the same values); append the frame and the scene
//   1  if the episode ends and has a slot: copy the rings out
//   2  the running state (lane 0); if the episode ends: s_0 of the next one
template <class Barrier>
MPC_HD void step_env(const Recorder &r, const StepInputs &in, int b, bool reset, int lane, int lanes, Barrier at) {
    const size_t B = (size_t)r.B;
    int32_t *si = r.state_i32 + b;
    if (reset) {
        if (lane == 0) {
            for (int f = 0; f < kStateI32; ++f) si[f * B] = 0;
            r.slot[b] = -1;
        }
        begin_episode(r, in.obs, b, lane, lanes);
        return;
    }
    const int32_t j = si[kOrdinal * B];
    if (j >= r.Q) return;                                    // the quota is recorded: steps with the batch, writes nothing
    const int32_t t = si[kSteps * B], oc = outcome_now(r, in, b), s = r.slot[b];
    const bool done = in.done[b] != 0;
    append(r, in, b, t, lane, lanes);
    at(0);
    if (done && s >= 0 && s < r.C) commit(r, b, s, t + 1, j, oc, lane, lanes);
    at(1);
    if (lane == 0) {
        si[kSteps * B] = done ? 0 : t + 1;
        si[kCrashed * B] = done ? 0 : (oc & kCollision ? 1 : 0);
        si[kUnsolved * B] = done ? 0 : (oc & kUnsolvedBit ? 1 : 0);
        if (done) si[kOrdinal * B] = j + 1;
    }
    if (done) begin_episode(r, in.obs, b, lane, lanes);
}

}  // namespace trace
}  // namespace mpc
