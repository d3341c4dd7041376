// Counted vector-memory waits of the register-tile k-loops (edge_gemm1_body, edge_gemm2b_kernel, gemm_rt_kernel: csrc/edge_stage.hip), from the
// first iteration to the last.
//
// The loop, per wave (P = LDS-DMA pieces per k-tile, R = ring loads per k-step, D = ring depth in k-steps, KT k-tiles of two k-steps each):
//
//     prologue:      DMA k-tiles 0, 1, 2 (3 P operations, unconditionally), then ring slices 0 .. D - 1 (D R operations)
//     iteration k:   HEAD WAIT: DMA k-tile k has landed;  barrier;  DMA k-tile k + 3 (P operations) if k + 3 < KT;
//                    for s2 = 0, 1, with s = 2 k + s2:   RING WAIT: slice s has landed;  MFMAs;  ring slice s + D (R operations) if s + D < 2 KT
//
// Vector memory operations retire in order, so `s_waitcnt vmcnt(n)` guarantees an operation has landed iff at most n operations were issued by
// this wave after it and before the wait.  lw_head_wait / lw_ring_wait return exactly that number: the largest legal immediate.  A larger one
// under-waits silently, a smaller one only costs time.  scripts/loop_waits_host_check.cpp replays the issue order through an in-order queue
// and asserts at every wait point that the count suffices and that count + 1 would not.
//
// s_waitcnt takes an immediate, so the kernels run the first four and the last four iterations as unrolled code around a steady-state loop
// (lw_k_loop below).  Away from both ends the counts depend only on the distance from the nearer end: any KT >= 8 runs with the counts of
// the canonical KT = 12 (iterations 0 .. 3, a steady pair, iterations KT - 4 .. KT - 1); KT = 2, 4, 6, where the fill and the drain overlap,
// have their own unrolled forms.  lw_canon_k is that mapping; the host check goes through it, so what it proves is what the kernels run.
// The form is a TEMPLATE PARAMETER of the kernels (lw_form / lw_dispatch_form), not a branch inside one: the weight ring and the fragments
// are written by loads the compiler cannot see land, so a register copy between a request and its wait -- which the register allocator
// places where differently allocated paths meet -- would copy stale data.  One straight path per kernel leaves it nothing to reconcile.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MI_LW_HD __host__ __device__
#else
#define MI_LW_HD
#endif

namespace mi {

constexpr int LW_VMCNT_MAX = 63;   // (the 6-bit vmcnt field of gfx9)
constexpr int LW_CANON_KT = 12;

MI_LW_HD constexpr bool lw_dma_issued(int KT, int k) { return k + 3 < KT; }             // iteration k requests k-tile k + 3
MI_LW_HD constexpr bool lw_ring_issued(int D, int KT, int s) { return s + D < 2 * KT; }   // k-step s requests slice s + D

// operations this wave has issued when it reaches the head wait of iteration k
MI_LW_HD constexpr int lw_issued_at_head(int P, int R, int D, int KT, int k) {
    int n = 3 * P + D * R;
    for (int j = 0; j < k; ++j) n += (lw_dma_issued(KT, j) ? P : 0) + (lw_ring_issued(D, KT, 2 * j) ? R : 0) + (lw_ring_issued(D, KT, 2 * j + 1) ? R : 0);
    return n;
}
// ... when it reaches the ring wait of k-step s
MI_LW_HD constexpr int lw_issued_at_ring(int P, int R, int D, int KT, int s) {
    const int k = s >> 1;
    return lw_issued_at_head(P, R, D, KT, k) + (lw_dma_issued(KT, k) ? P : 0) + ((s & 1) && lw_ring_issued(D, KT, 2 * k) ? R : 0);
}
MI_LW_HD constexpr int lw_clamp(int n) { return n < 0 ? 0 : n > LW_VMCNT_MAX ? LW_VMCNT_MAX : n; }

// (i) head of iteration k: k-tile k's last piece was issued in the prologue (k < 3) or right behind the head wait of iteration k - 3
MI_LW_HD constexpr int lw_head_wait(int P, int R, int D, int KT, int k) {
    const int through = k < 3 ? (k + 1) * P : lw_issued_at_head(P, R, D, KT, k - 3) + P;
    return lw_clamp(lw_issued_at_head(P, R, D, KT, k) - through);
}
// (ii) ring wait of k-step s: slice s's last load was issued in the prologue (s < D) or right behind the ring wait of k-step s - D
MI_LW_HD constexpr int lw_ring_wait(int P, int R, int D, int KT, int s) {
    const int through = s < D ? 3 * P + (s + 1) * R : lw_issued_at_ring(P, R, D, KT, s - D) + R;
    return lw_clamp(lw_issued_at_ring(P, R, D, KT, s) - through);
}

// the iteration of the canonical loop whose counts (and issue decisions) iteration k of a KT-tile loop runs with
MI_LW_HD constexpr int lw_canon_kt(int KT) { return KT >= 8 ? LW_CANON_KT : KT; }
MI_LW_HD constexpr int lw_canon_k(int KT, int k) { return KT < 8 ? k : k < 4 ? k : k >= KT - 4 ? k - KT + LW_CANON_KT : 4 + (k & 1); }

template <int V>
struct LwInt {
    static constexpr int value = V;
};
// the unrolled form a KT-tile loop runs: 0 = the general one (KT >= 8), else KT itself (2, 4, 6); the host picks the kernel instance with it
constexpr int lw_form(int KT) { return KT >= 8 ? 0 : KT; }
template <class F>
inline auto lw_dispatch_form(int KT, F&& f) {
    switch (lw_form(KT)) {
        case 0: return f(LwInt<0>{});
        case 6: return f(LwInt<6>{});
        case 4: return f(LwInt<4>{});
        default: return f(LwInt<2>{});
    }
}

#if defined(__HIPCC__)
// One iteration with compile-time counts.  head(k, HW, DMA, MARK): the head wait vmcnt(HW), the barrier, the request of k-tile k + 3 iff DMA;
// MARK tells the phase clock the first iteration and the third from the end.  step(k, SLOT, RW, ISSUE): k-step 2 k + (SLOT & 1) on ring slot
// SLOT behind vmcnt(RW), the request of slice + D iff ISSUE.  k is the true iteration (addresses), KC the canonical one (counts).
constexpr int LW_MARK_FIRST = 1, LW_MARK_TAIL = 2;
template <int P, int R, int D, int KTC, int KC, class Head, class Step>
__device__ __forceinline__ void lw_iter(int k, Head& head, Step& step) {
    head(k, LwInt<lw_head_wait(P, R, D, KTC, KC)>{}, LwInt<lw_dma_issued(KTC, KC)>{}, LwInt<(KC == 0 ? LW_MARK_FIRST : KC == KTC - 3 ? LW_MARK_TAIL : 0)>{});
    step(k, LwInt<2 * (KC & 1)>{}, LwInt<lw_ring_wait(P, R, D, KTC, 2 * KC)>{}, LwInt<lw_ring_issued(D, KTC, 2 * KC)>{});
    step(k, LwInt<2 * (KC & 1) + 1>{}, LwInt<lw_ring_wait(P, R, D, KTC, 2 * KC + 1)>{}, LwInt<lw_ring_issued(D, KTC, 2 * KC + 1)>{});
}
template <int P, int R, int D, int KTC, int KC, class Head, class Step>
__device__ __forceinline__ void lw_pair(int kt, Head& head, Step& step) {
    lw_iter<P, R, D, KTC, KC>(kt, head, step);
    lw_iter<P, R, D, KTC, KC + 1>(kt + 1, head, step);
}

// the whole k-loop of a kernel instance of form FORM (KT even, lw_form(KT) == FORM)
template <int P, int R, int D, int FORM, class Head, class Step>
__device__ __forceinline__ void lw_k_loop(int KT, Head& head, Step& step) {
    static_assert(D == 4, "two k-tiles of ring per pair of iterations");
    static_assert(FORM == 0 || FORM == 2 || FORM == 4 || FORM == 6, "the general form or one of the short ones");
    static_assert(lw_canon_k(8, 3) == 3 && lw_canon_k(8, 4) == 8 && lw_canon_k(10, 4) == 4 && lw_canon_k(10, 5) == 5 && lw_canon_k(10, 6) == 8, "canonical iterations");
    if constexpr (FORM == 0) {
        lw_pair<P, R, D, LW_CANON_KT, 0>(0, head, step);
        lw_pair<P, R, D, LW_CANON_KT, 2>(2, head, step);
#pragma unroll 1
        for (int kt = 4; kt < KT - 4; kt += 2) lw_pair<P, R, D, LW_CANON_KT, 4>(kt, head, step);
        lw_pair<P, R, D, LW_CANON_KT, 8>(KT - 4, head, step);
        lw_pair<P, R, D, LW_CANON_KT, 10>(KT - 2, head, step);
    } else {
        lw_pair<P, R, D, FORM, 0>(0, head, step);
        if constexpr (FORM >= 4) lw_pair<P, R, D, FORM, 2>(2, head, step);
        if constexpr (FORM >= 6) lw_pair<P, R, D, FORM, 4>(4, head, step);
    }
}
#endif

}  // namespace mi
