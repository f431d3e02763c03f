// The two-threshold detector's state machine on predicate words (VAD_detection, VAD.py:136-182), shared by vad_detect_kernel (vad.hip)
// and vad_sweep_kernel (vad_sweep.hip): one wave runs it on three planes of 64-frame words — loud (power > amph), active (power > ampl
// or zcr > zcr_gate) and the mark plane it fills.  Bits at and above the utterance's length are clear in every plane.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace ssp {

__device__ __forceinline__ uint64_t ldw(const uint64_t* p) {  // a word every lane reads from the same address, as a wave-uniform value
    const uint64_t v = *p;
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}
// first index >= i whose bit is set (FLIP: clear), n if none.  Bits at and above n are clear in every plane.
template <bool FLIP>
__device__ __forceinline__ int vad_next(const uint64_t* P, int i, int n) {
    if (i >= n) return n;
    const int nw = (n + 63) >> 6;
    int w = i >> 6;
    uint64_t x = (FLIP ? ~ldw(P + w) : ldw(P + w)) & (~0ull << (i & 63));
    while (x == 0) {
        if (++w >= nw) return n;
        x = FLIP ? ~ldw(P + w) : ldw(P + w);
    }
    const int r = w * 64 + __builtin_ctzll(x);
    return r < n ? r : n;
}
// last index <= i whose bit is clear, -1 if none
__device__ __forceinline__ int vad_prev_clear(const uint64_t* P, int i) {
    int w = i >> 6;
    uint64_t x = ~ldw(P + w) & (~0ull >> (63 - (i & 63)));
    while (x == 0) {
        if (--w < 0) return -1;
        x = ~ldw(P + w);
    }
    return w * 64 + 63 - __builtin_clzll(x);
}

// The reference's loop, frame by frame: a loud frame extends the run (end = i) and opens one if none is open (start = i); any
// other frame flushes the run if it is longer than min_len: start walks back and end forward over active frames, [start, end] is
// marked, the run is closed.  A run that is too short stays OPEN with its start (a later loud frame extends it across the gap);
// a run still open at the last frame is never flushed.  Runs of loud frames and the two walks are bit searches here.
// Not implemented: the last_end / min_distance merge (VAD.py:172-174) — last_end starts at -1 and is only set inside the branch
// that needs it positive, so the branch is never taken.  Deviation: the backward walk stops at frame 0, where Python's index -1
// would go on with the LAST frame (the same result whenever the last frame is not active).
// L, A: the loud and active words of T frames, visible to the whole wave; M: zeroed by the caller, ORed with the marks (lane-parallel
// over words).  Every lane of the wave calls it with the same arguments.
__device__ __forceinline__ void vad_mark_runs(const uint64_t* L, const uint64_t* A, uint64_t* M, int T, int min_len, int lane) {
    int i = 0, start = 0;
    bool open = false;
    for (;;) {
        const int jn = vad_next<false>(L, i, T);
        if (jn >= T) break;
        if (!open) start = jn, open = true;
        const int k = vad_next<true>(L, jn, T);  // first frame behind the loud streak
        if (k >= T) break;
        const int end = k - 1;
        if (end - start + 1 > min_len) {
            const int st = vad_prev_clear(A, start) + 1;
            const int en = vad_next<true>(A, end, T) - 1;
            for (int w = (st >> 6) + lane; w <= (en >> 6) && st <= en; w += 64) {
                const int lo = w == (st >> 6) ? (st & 63) : 0, hi = w == (en >> 6) ? (en & 63) : 63;
                M[w] |= (~0ull << lo) & (~0ull >> (63 - hi));
            }
            __threadfence_block();
            open = false;
        }
        i = k + 1;
    }
}

}  // namespace ssp
