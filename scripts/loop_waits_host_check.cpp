// The counted waits of the register-tile k-loops (matinvent_amd/csrc/loop_waits.h: the vmcnt immediates that edge_gemm1_body,
// edge_gemm2b_kernel and gemm_rt_kernel run with from their first iteration to their last) proved on the host: each loop's issue order is
// replayed through an in-order queue of vector-memory operations, and at every wait point
//   (a) the awaited operation has retired once the queue is cut to the returned count, both with the waits in front of it applied and with
//       none of them applied (every operation issued so far still in flight: the worst case for this wait alone);
//   (b) cut to count + 1, in that worst case, the awaited operation is still in flight: the wait is tight;
//   (c) the issue decisions of the canonical iteration the kernel runs (lw_canon_k) are those of the true iteration.
// The counts are taken the way the kernels take them: through lw_canon_kt / lw_canon_k.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/loop_waits_host_check.cpp -o loop_waits_host_check
//   ./loop_waits_host_check
//
// Cases: edge_gemm1b (4 DMA pieces, 2 ring loads) at KT = 2, 4, 6, 8, 24; edge_gemm2b (4, 4) at KT = 16; gemm_rt (4, 4) at KT = 2, 4, 6, 16, 32;
// and every even KT up to 64 of both shapes.  Exit status 0: every wait point of every case holds; 1: a violation (printed).
#include <cstdio>
#include <deque>
#include <vector>

#include "../matinvent_amd/csrc/loop_waits.h"

using namespace mi;

struct Queue {
    std::deque<int> q;   // operations in flight, oldest first: they retire in order
    int next = 0;
    int issue(int n) {   // returns the id of the last one issued
        for (int i = 0; i < n; ++i) q.push_back(next++);
        return next - 1;
    }
    void wait(int cnt) {
        while ((int)q.size() > cnt) q.pop_front();
    }
    bool in_flight(int id) const { return !q.empty() && id >= q.front(); }
};

static int waits_checked = 0;

// one wait point: `live` carries the waits in front of it, `awaited` the id that must have landed
static int wait_point(Queue& live, int awaited, int cnt, const char* loop, int KT, const char* what, int idx) {
    int bad = 0;
    ++waits_checked;
    Queue alone;   // no earlier wait applied: everything issued so far in flight
    alone.issue(live.next);
    Queue loose = alone;
    alone.wait(cnt);
    loose.wait(cnt + 1);
    live.wait(cnt);
    if (live.in_flight(awaited) || alone.in_flight(awaited)) {
        printf("%s KT=%d %s %d: vmcnt(%d) UNDER-WAITS (operation %d of %d still in flight)\n", loop, KT, what, idx, cnt, awaited, live.next);
        ++bad;
    }
    if (cnt < LW_VMCNT_MAX && !loose.in_flight(awaited)) {
        printf("%s KT=%d %s %d: vmcnt(%d) is not tight (vmcnt(%d) would do)\n", loop, KT, what, idx, cnt, cnt + 1);
        ++bad;
    }
    return bad;
}

static int replay(const char* loop, int P, int R, int D, int KT, bool print) {
    int bad = 0;
    const int KS = 2 * KT, KTC = lw_canon_kt(KT);
    Queue q;
    std::vector<int> dma_last(KT + 3, -1), ring_last(KS + D, -1);
    for (int t = 0; t < 3; ++t) dma_last[t] = q.issue(P);   // (k-tiles 1, 2 are requested whatever KT is)
    for (int d = 0; d < D; ++d) ring_last[d] = q.issue(R);
    if (print) printf("%s KT=%d:", loop, KT);
    for (int k = 0; k < KT; ++k) {
        const int kc = lw_canon_k(KT, k);
        const int hw = lw_head_wait(P, R, D, KTC, kc);
        if (print) printf("  [%d] h%d", k, hw);
        bad += wait_point(q, dma_last[k], hw, loop, KT, "head of iteration", k);
        if (lw_dma_issued(KTC, kc) != (k + 3 < KT)) {
            printf("%s KT=%d iteration %d: canonical iteration %d of %d decides the DMA request differently\n", loop, KT, k, kc, KTC);
            ++bad;
        }
        if (k + 3 < KT) dma_last[k + 3] = q.issue(P);
        for (int s2 = 0; s2 < 2; ++s2) {
            const int s = 2 * k + s2;
            const int rw = lw_ring_wait(P, R, D, KTC, 2 * kc + s2);
            if (print) printf(" r%d", rw);
            bad += wait_point(q, ring_last[s], rw, loop, KT, "ring wait of k-step", s);
            if (lw_ring_issued(D, KTC, 2 * kc + s2) != (s + D < KS)) {
                printf("%s KT=%d k-step %d: canonical iteration %d of %d decides the ring request differently\n", loop, KT, s, kc, KTC);
                ++bad;
            }
            if (s + D < KS) ring_last[s + D] = q.issue(R);
        }
    }
    if (print) printf("\n");
    q.wait(0);
    return bad;
}

// the steady state, worked by hand: a slice has the other three slices and two k-tile heads behind it (3 R + 2 P); a k-tile's last piece has
// three iterations' ring loads and two later heads behind it (6 R + 2 P).  (The head waits ran with 16 and 24 before the whole loop was
// counted: "at least" that many, on the safe side.)
static_assert(lw_head_wait(4, 2, 4, 12, 4) == 20 && lw_ring_wait(4, 2, 4, 12, 8) == 14 && lw_ring_wait(4, 2, 4, 12, 9) == 14, "edge_gemm1b steady state");
static_assert(lw_head_wait(4, 4, 4, 12, 5) == 32 && lw_ring_wait(4, 4, 4, 12, 10) == 20 && lw_ring_wait(4, 4, 4, 12, 11) == 20, "edge_gemm2b / gemm_rt steady state");
// the last ring wait of a loop has nothing behind it
static_assert(lw_ring_wait(4, 2, 4, 12, 23) == 0 && lw_ring_wait(4, 4, 4, 2, 3) == 0, "last k-step");

int main() {
    int bad = 0, cases = 0;
    for (int KT : {2, 4, 6, 8, 24}) bad += replay("edge_gemm1b", 4, 2, 4, KT, true), ++cases;
    bad += replay("edge_gemm2b", 4, 4, 4, 16, true), ++cases;
    for (int KT : {2, 4, 6, 16, 32}) bad += replay("gemm_rt", 4, 4, 4, KT, true), ++cases;
    for (int KT = 2; KT <= 64; KT += 2) {
        bad += replay("edge_gemm1b", 4, 2, 4, KT, false);
        bad += replay("gemm_rt", 4, 4, 4, KT, false);
        cases += 2;
    }
    printf("%d cases, %d wait points, %d violations\n", cases, waits_checked, bad);
    return bad ? 1 : 0;
}
