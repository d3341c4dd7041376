// Second linear of the edge MLP with the edge -> node reduction, inference form (cspnet.py:73-79):
//
//     M2 = SiLU(M1 W2^T + b2)   over the E directed edges (rows in CSR order: sorted by source node),
//     part[slot][node] = sum of the node's rows inside one 128-row tile       (finalize / node chain: sum of slots / degree)
//
// What differs from the 128 x 128-tile plane GEMM (gemm_split.h) that runs this product everywhere else:
//   * a four-wave workgroup owns 128 rows and 256 of the H = 512 output columns, its fp32 accumulators in registers (128 per lane): the A
//     operand (the M1 planes) comes from HBM once and from L2 once instead of once per 128-column tile, and a wave multiplies 4 x 2 MFMA
//     tiles per fragment set -- 8 LDS fragment reads per 24 MFMAs instead of 8 per 12;
//   * the W operand never touches LDS: a weight element is used by exactly one wave of the workgroup, so the weights come pre-split in
//     MFMA FRAGMENT ORDER straight from L2 into a register ring (node_chain.hip's scheme);
//   * the A operand streams through four 16 KiB LDS stages of one 32-deep k-tile each by LDS-DMA (`buffer_load ... lds`), the XOR swizzle
//     applied on the source side;
//   * the segmented row sum is an MFMA product too:  part = S x M2  with S[node][row] = 1 iff the row's source is that node.  In the MFMA
//     result layout a lane owns one column of 4 x 4 rows -- exactly a B-operand fragment once the rows' k order is permuted, which the
//     0/1 matrix S absorbs -- so SiLU(M2) is split into its two fp16 planes in registers and multiplied by S (exact), instead of the
//     per-run select-and-add loops over 16 registers that made the epilogue a quarter of the old kernel.
// Same plane format, same scales, same three-term products in the same k order as the plane GEMM: M2 agrees to fp32 round-off; the
// partial sums additionally round M2 to the 22 bits of the plane format (scale = the rigorous bound of |Z2| the layer's aggregated
// messages use anyway).
#include <mutex>

#include <cstdio>
#include <cstdlib>
#include "net.h"
#include "gemm_split.h"
#include "loop_waits.h"
// The k-loops of edge_gemm1b_kernel, edge_gemm2b_kernel and gemm_rt_kernel run with EVERY memory operation under manual control: LDS fragment
// reads and the weight ring as inline asm with counted lgkmcnt / vmcnt waits, and a bare s_barrier.  With compiler-visible LDS reads and
// __syncthreads() the compiler drains the LDS-DMA in flight in front of every barrier (`s_waitcnt vmcnt(1)`: it cannot tell that the k-tiles
// requested two and three iterations ahead target other stages than the one being read).  (Those forms measured 1-4 % slower: docs/rounds/round4.md
// 18.4e, profiles/r4_asm_lds_ab.log; last present at 3e3d930.)
#define MI_LOOP_BARRIER() __builtin_amdgcn_s_barrier()
// Phase-clock stamp inside a k-loop, at an iteration's head (no LDS read in flight there): the clock read with its own wait in ONE statement --
// s_memtime returns out of order with LDS reads, so left pending it would blur the loop's counted lgkmcnt waits -- into scalar registers; the
// kernel stores them behind the loop (a store inside it would only be one more operation behind everything in flight: a wait too early).
#define MI_LOOP_STAMP(t) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory")
// Weight slice of a k-step: requested four steps ahead; vector loads retire in order, so it has arrived once no more operations are outstanding
// than this wave issued behind it -- in the steady state the other three slices in flight and the LDS-DMA pieces of the two k-tile heads in
// between, fewer while the loop fills and drains (loop_waits.h has the count for every k-step).  The slice rides through the wait as
// read-write operands, so that no MFMA can be scheduled in front of it.
#define MI_RING_WAIT(w, n) asm volatile("s_waitcnt vmcnt(%4)" : "+v"((w)[0][0]), "+v"((w)[0][1]), "+v"((w)[1][0]), "+v"((w)[1][1]) : "n"(n))

namespace mi {

extern int g_edge2_train;
int g_edge2_fused = 1;   // inference forwards at hidden_dim 512: the second edge GEMM on the 128 x 256 register-tile kernel (0: plane GEMM)

#if MI_PLANES_FP16

struct EdgeGemm2Args {
    Planes A;                 // M1 planes [E x H] (tile-blocked, scale dsc[0])
    const u16* W2f;           // fragment-order pack of edge_mlp.2.weight [H x H]
    const float* b2;
    const float* dsc;         // {s_M1, 1/s_M1, s_agg, 1/s_agg, ...} (act_scales_eval)
    const int* src;           // [E] source node of each row
    const int* rowptr;        // [N + 1]
    float* part;              // [nslots][N][H], slot = tile - (first row of the node >> 7)
    int E, N;
    const int* tab = nullptr; // [tiles][EG2_TAB] per-tile tables {first node, local nodes, srcl[128], slotb[128]} (edge2_tables_kernel; edge_gemm2b_kernel)
    float* Z2 = nullptr;      // optional (training forward): the pre-activation M1 W2^T + b2, fp32 [E][H], kept for the backward pass
    unsigned long long* clk;  // optional phase clock: [tile][8] s_memtime stamps (mi_debug_edge2_clock)
};

// Per-tile tables of the second edge GEMM (a 128-row tile's first source node, its number of local nodes, each row's local source index and each
// local node's slot): a function of the edge list alone, so they are built ONCE per graph (fc: once per batch; knn: once per forward) instead of
// by every workgroup of every layer -- where they were a chain of three dependent loads, each behind an s_waitcnt vmcnt(0) that also waited for
// the twelve LDS-DMA pieces and the weight ring issued in front of it, plus one more at the head of the epilogue (ISA).
constexpr int EG2_TAB = 2 + 128 + 128;
__global__ __launch_bounds__(128) void edge2_tables_kernel(const int* __restrict__ src, const int* __restrict__ rowptr, int E, int N, int* __restrict__ tab) {
    const int tile = blockIdx.x, tid = threadIdx.x, row0 = tile * 128;
    if (row0 >= E) return;
    const int nrows = E - row0 < 128 ? E - row0 : 128;
    const int node_first = src[row0];
    int* t = tab + (size_t)tile * EG2_TAB;
    const int r = row0 + tid, node = node_first + tid;
    t[2 + tid] = r < E ? src[r] - node_first : -1;
    t[130 + tid] = node < N ? tile - (rowptr[node] >> 7) : 0;
    if (tid == 0) {
        t[0] = node_first;
        t[1] = src[row0 + nrows - 1] - node_first + 1;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Form B: 128 rows x 256 columns per FOUR-wave workgroup, TWO workgroups per CU.  A wave owns 4 x 2 MFMA tiles (128 accumulator
// registers, its weights straight from L2).  The two workgroups of a CU are independent, so they drift apart and one's epilogue -- SiLU
// and the plane split are ~11k VALU cycles per wave -- runs under the other's MFMA loop; so do the operand fills at a tile's start.  (In
// the eight-wave 128 x 512 form that this one replaced both waves of a SIMD reached the epilogue together, a quarter of a tile's time:
// docs/rounds/round3.md 16.3; last present at 3e3d930.)  The A operand goes through four 16 KiB LDS stages of one 32-deep k-tile each
// (the plane GEMM's LDS image and source-side swizzle), three k-tiles ahead; the two column halves of a row tile run on the same XCD
// (its second read of A hits L2).
// ------------------------------------------------------------------------------------------------------------------------------------
constexpr int EG2B_STAGE = 2 * 128 * 64, EG2B_NST = 4;                   // [plane][row 128][32 k halfs]
constexpr int EG2B_LDS = EG2B_NST * EG2B_STAGE + 128 * 4 + 128 * 4;      // stages (overlaid by the S fragments in the epilogue) + srcl + slotb

template <int D, bool SAVE_Z = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void edge_gemm2b_kernel(EdgeGemm2Args a) {
    constexpr int H = 512, KS = H / 16, KT = H / 32;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int* srcl = reinterpret_cast<int*>(smem + EG2B_NST * EG2B_STAGE);
    int* slotb = srcl + 128;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, kg = lane >> 5;
    // XCD-aware mapping (workgroups go round-robin to the 8 XCDs): both column halves of a row tile on the same XCD
    const int id = blockIdx.x, slot = id >> 3, half = slot & 1, tile = (slot >> 1) * 8 + (id & 7);
    const int row0 = tile * 128;
    if (row0 >= a.E) return;
    const int nrows = a.E - row0 < 128 ? a.E - row0 : 128;
    int stamp_i = 0;
    auto stamp = [&]() {
        if (a.clk && tid == 0) a.clk[(size_t)(tile * 2 + half) * 8 + stamp_i] = __builtin_amdgcn_s_memtime();
        ++stamp_i;
    };
    stamp();
    if (a.clk && tid == 0) a.clk[(size_t)(tile * 2 + half) * 8 + 4] = __builtin_amdgcn_s_memrealtime();   // (100 MHz: stamps 4 / 5 give the shader clock the other four ran at)

    // per-tile tables (edge2_tables_kernel), requested FIRST: independent loads that land under the operand stream; consumed after it is issued
    const int* tab = a.tab + (size_t)tile * EG2_TAB;
    int t_srcl = -1, t_slotb = 0;
    if (tid < 128) {
        t_srcl = tab[2 + tid];
        t_slotb = tab[130 + tid];
    }
    const int node_first = tab[0], cnt_tab = tab[1];

    // ---- A operand: k-tile kt = one 16 KiB block [plane][128 rows][64 B] of the plane set, 16 pieces of 1 KiB, four per wave ----
    // LDS image of a stage = the plane GEMM's: 64-byte rows, 16-byte piece c of row r at position c ^ ((r >> 2) & 3)
    const __amdgpu_buffer_rsrc_t rsa = uniform_rsrc(a.A.base + a.A.tile(tile, 0), a.A.KT * 24576);
    const int voffa = (lane >> 2) * 64 + (((lane & 3) ^ ((lane >> 4) & 3)) << 4);
    auto dma_tile = [&](int kt, int st) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int piece = wave * 4 + q;   // plane = piece >> 3, rows 16 (piece & 7) .. + 15
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsa, (__attribute__((address_space(3))) void*)(smem + st * EG2B_STAGE + piece * 1024), 16, voffa,
                                                     kt * 24576 + (piece >> 3) * 8192 + (piece & 7) * 1024, 0, 0);   // (aux 2 = non-temporal measured no gain: DESIGN 19.7)
        }
    };
    dma_tile(0, 0);
    dma_tile(1, 1);
    dma_tile(2, 2);

    // ---- W operand: register ring over the k-steps, the wave's two column tiles: columns 256 half + 64 wave .. + 63 ----
    int voffw[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) voffw[t] = lane * 16 + ((8 * half + 2 * wave + t) * KS) * 2048;
    u32x4 ring[D][2][2];
    // (inline asm, with a counted wait in front of every step's MFMAs: see MI_RING_WAIT)
    const u32x4 rsw_s = rsrc_words(a.W2f, H * H * 4);
    auto ring_load = [&](int ks, u32x4 (&w)[2][2]) {
        const int soff = __builtin_amdgcn_readfirstlane(ks * 2048);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(w[t][0]) : "v"(voffw[t]), "s"(rsw_s), "s"(soff));
            asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen offset:1024" : "=v"(w[t][1]) : "v"(voffw[t]), "s"(rsw_s), "s"(soff));
        }
    };
    // (inside the loop the slot is a read-write operand of its own reload: the slice stays in the registers the prologue gave it, from the
    //  first request to the last product -- no new value for the register allocator to place somewhere else)
    auto ring_reload = [&](int ks, u32x4 (&w)[2][2]) {
        const int soff = __builtin_amdgcn_readfirstlane(ks * 2048);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "+v"(w[t][0]) : "v"(voffw[t]), "s"(rsw_s), "s"(soff));
            asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen offset:1024" : "+v"(w[t][1]) : "v"(voffw[t]), "s"(rsw_s), "s"(soff));
        }
    };
#pragma unroll
    for (int d = 0; d < D; ++d) ring_load(d, ring[d]);

    if (tid < 128) {   // (the tables were requested before the operand loads: this waits for them alone)
        srcl[tid] = t_srcl;
        slotb[tid] = t_slotb;
    }
    const float os = a.dsc[1] * (1.f / PL_SW), s_m2 = a.dsc[2], inv_m2 = a.dsc[3];

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // The fragment reads as inline asm with their own lgkmcnt wait, and the bare s_barrier instead of __syncthreads(): the compiler cannot tell
    // that the LDS-DMA in flight targets other stages than the one being read, so it drains it -- in this loop `s_waitcnt vmcnt(1)` in front of
    // every barrier, i.e. the k-tiles requested two and three iterations ahead had to LAND before the current one was used (found in
    // gemm_tn_planes_kernel, backward.hip, where the same cost 30 %).  The fragments ride through the wait as read-write operands, so that no
    // MFMA can be scheduled in front of it.
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
    unsigned rd_off[2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) rd_off[s2] = lds0 + (unsigned)(l31 * 64 + (((2 * s2 + kg) ^ ((l31 >> 2) & 3)) * 16));
    auto read_a = [&](int st, int s2, f16x8 (&af)[4][2]) {
        const unsigned va = rd_off[s2] + (unsigned)st * EG2B_STAGE;
#define MI_RD128(dst, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(va), "n"(off))
        MI_RD128(af[0][0], 0 * 2048);        MI_RD128(af[0][1], 0 * 2048 + 8192);
        MI_RD128(af[1][0], 1 * 2048);        MI_RD128(af[1][1], 1 * 2048 + 8192);
        MI_RD128(af[2][0], 2 * 2048);        MI_RD128(af[2][1], 2 * 2048 + 8192);
        MI_RD128(af[3][0], 3 * 2048);        MI_RD128(af[3][1], 3 * 2048 + 8192);
#undef MI_RD128
        // (no wait here: the lgkmcnt waits in front of the MFMAs that read the fragments -- LDS reads return in order, so the first two row blocks' four
        //  reads are complete when at most four are outstanding)
    };
    auto mma = [&](const u32x4 (&w)[2][2], f16x8 (&af)[4][2]) {   // terms (a1, b0), (a0, b1), (a0, b0): the plane GEMM's order; two row blocks at a time, each pair behind the wait for its own fragments
#pragma unroll
        for (int ip = 0; ip < 2; ++ip) {
            if (ip == 0) asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(af[0][0]), "+v"(af[0][1]), "+v"(af[1][0]), "+v"(af[1][1]));
            else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(af[2][0]), "+v"(af[2][1]), "+v"(af[3][0]), "+v"(af[3][1]));
#pragma unroll
            for (int term = MI_TERM0; term < 3; ++term)
#pragma unroll
                for (int i = 2 * ip; i < 2 * ip + 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i][term == 0 ? 1 : 0], __builtin_bit_cast(f16x8, w[j][term == 1 ? 1 : 0]), acc[i][j], 0, 0, 0);
        }
    };
    static_assert(D == 4, "two k-tiles of ring per unrolled pair of iterations");
    // Every wait of the loop is counted, from the fill to the drain (loop_waits.h: per k-tile this wave issues 4 DMA pieces -- k-tile k + 3 --
    // and then 2 x 4 ring loads; a k-tile or a slice has landed once no more operations are outstanding than were issued behind it).  The
    // phase clock keeps its two in-loop stamps in scalar registers and stores them behind the loop (MI_LOOP_STAMP).
    unsigned long long t_first = 0, t_tail = 0;
    auto head = [&](int k, auto hw, auto dma, auto mark) {
        if (decltype(mark)::value == LW_MARK_TAIL && a.clk) MI_LOOP_STAMP(t_tail);   // head of the third iteration from the end
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(decltype(hw)::value) : "memory");
        MI_LOOP_BARRIER();   // k-tile k has landed for every wave; every wave is done with the stage k-tile k + 3 goes to (= that of k - 1)
        if (decltype(mark)::value == LW_MARK_FIRST && a.clk) MI_LOOP_STAMP(t_first);
        if (decltype(dma)::value) dma_tile(k + 3, (k + 3) & 3);
    };
    auto step = [&](int k, auto slot, auto rw, auto issue) {
        constexpr int SL = decltype(slot)::value, s2 = SL & 1;
        f16x8 af[4][2];
        read_a(k & 3, s2, af);
        MI_RING_WAIT(ring[SL], decltype(rw)::value);
        mma(ring[SL], af);
        if (decltype(issue)::value) ring_reload(2 * k + s2 + D, ring[SL]);
        __builtin_amdgcn_sched_barrier(0);
    };
    lw_k_loop<4, 4, D, lw_form(KT)>(KT, head, step);
    stamp_i = 2;
    stamp();
    if (a.clk && tid == 0) {
        a.clk[(size_t)(tile * 2 + half) * 8 + 1] = t_first;
        a.clk[(size_t)(tile * 2 + half) * 8 + 6] = t_tail;
    }

    if constexpr (SAVE_Z) {
        // training forward: Z2 = acc / (s_A s_W) + b2 is kept for the backward pass.  In the result layout that would be 128 four-byte
        // stores per lane; through a per-wave LDS patch (the plane GEMM's planes_store_preact_rows) every store is a 16-byte row-major piece.
        __syncthreads();   // every wave is out of the main loop: the patches overlay the operand stages
        float* stage = reinterpret_cast<float*>(smem) + wave * 1152;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int rb = row0 + i * 32, cb = half * 256 + wave * 64 + j * 32;
#pragma unroll
                for (int r = 0; r < 16; ++r) stage[((r & 3) + 8 * (r >> 2) + 4 * kg) * 36 + l31] = acc[i][j][r] * os;
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int q = lane + 64 * u, rl = q >> 2, c8 = (q & 3) * 8;
                    const int row = rb + rl, col = cb + c8;
                    f32x4 z0 = *reinterpret_cast<const f32x4*>(stage + rl * 36 + c8);
                    f32x4 z1 = *reinterpret_cast<const f32x4*>(stage + rl * 36 + c8 + 4);
                    if (row < a.E) {
                        z0 += *reinterpret_cast<const f32x4*>(a.b2 + col);
                        z1 += *reinterpret_cast<const f32x4*>(a.b2 + col + 4);
                        float* d = a.Z2 + (size_t)row * H + col;
                        *reinterpret_cast<f32x4*>(d) = z0;
                        *reinterpret_cast<f32x4*>(d + 4) = z1;
                    }
                }
                __builtin_amdgcn_wave_barrier();
            }
    }

    // ---- epilogue: M2 = SiLU(acc / (s_A s_W) + b2) -> two fp16 planes in registers -> part = S x M2 on the matrix pipe ----
    // k order of a 32-row block's two k-steps (u = 0, 1): lane group kg holds rows 4 kg + 8 (2 u + (idx >> 2)) + (idx & 3), idx = 0 .. 7.
    // The S fragments -- S[32 lb + l31][those rows] = 1 iff the row's local source is that node -- are the same for every wave and both
    // column tiles: built once into LDS in fragment order, [block][rb][u][lane][8 halfs] (8 KiB per 32-node block, overlays the operand
    // stages), and read back with one ds_read_b128 each.
    const int cnt = nrows > 0 ? cnt_tab : 0;
    u16* sfr = reinterpret_cast<u16*>(smem);
    unsigned sat = 0;
    const int nlb = (cnt + 31) >> 5;
    __syncthreads();
    for (int f = tid; f < nlb * 8 * 64; f += 256) {
        const int ln = f & 63, fu = (f >> 6) & 1, frb = (f >> 7) & 3, fq = f >> 9;   // one (fragment, lane) per iteration: 16 bytes
        const int me = fq * 32 + (ln & 31), fkg = ln >> 5;
        u32x4 w;
#pragma unroll
        for (int i2 = 0; i2 < 4; ++i2) {
            const int ia = 2 * i2, ib = 2 * i2 + 1;
            const int ra = frb * 32 + 4 * fkg + 8 * (2 * fu + (ia >> 2)) + (ia & 3), rbb = frb * 32 + 4 * fkg + 8 * (2 * fu + (ib >> 2)) + (ib & 3);
            w[i2] = (srcl[ra] == me ? 0x3C00u : 0u) | (srcl[rbb] == me ? 0x3C000000u : 0u);
        }
        *reinterpret_cast<u32x4*>(sfr + (size_t)f * 8) = w;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        __builtin_amdgcn_sched_barrier(0);
        const int col = half * 256 + wave * 64 + j * 32 + l31;
        const float bcol = a.b2[col];
#pragma unroll 1
        for (int lb0 = 0; lb0 < nlb; lb0 += 2) {
            const bool two = lb0 + 1 < nlb;
            f32x16 ps[2];
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r) ps[q][r] = 0.f;
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) {
                const f32x16 av = acc[rb][j];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    f16x8 mh, ml;
#pragma unroll
                    for (int idx = 0; idx < 8; idx += 2) {
                        const float v0 = silu_fast(av[8 * u + idx] * os + bcol), v1 = silu_fast(av[8 * u + idx + 1] * os + bcol);
                        unsigned p[3];
                        pl_split_pair_acc(v0, v1, s_m2, p, sat);
                        const f16x2 h = __builtin_bit_cast(f16x2, p[0]), lo = __builtin_bit_cast(f16x2, p[1]);
                        mh[idx] = h[0]; mh[idx + 1] = h[1];
                        ml[idx] = lo[0]; ml[idx + 1] = lo[1];
                    }
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        if (q == 1 && !two) break;
                        const f16x8 sf = *reinterpret_cast<const f16x8*>(sfr + (size_t)((((lb0 + q) * 4 + rb) * 2 + u) * 64 + lane) * 8);
                        ps[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(sf, ml, ps[q], 0, 0, 0);
                        ps[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(sf, mh, ps[q], 0, 0, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int loc = (lb0 + q) * 32 + (r & 3) + 8 * (r >> 2) + 4 * kg;
                    if (loc < cnt) a.part[((size_t)slotb[loc] * a.N + node_first + loc) * H + col] = ps[q][r] * inv_m2;
                }
        }
    }
    stamp();
    if (a.clk && tid == 0) a.clk[(size_t)(tile * 2 + half) * 8 + 5] = __builtin_amdgcn_s_memrealtime();
    sat_report(sat);
}

// ------------------------------------------------------------------------------------------------------------------------------------
// The same main loop as a general product  C = epilogue(A W^T)  with the plane GEMM's row-major epilogue (gemm_rt, picked by
// gemm_planes for operands that carry a fragment-order W): 128 rows x 256 columns per four-wave workgroup, any K % 64 == 0, any
// N % 256 == 0; the column blocks of a row tile run on the same XCD.  Same products, same k order, same epilogue function as the
// 128 x 128 plane kernel: bit-identical results.
// ------------------------------------------------------------------------------------------------------------------------------------
template <bool EXT, bool LEAN, int FORM>   // FORM: the unrolled form of the k-loop (loop_waits.h lw_form: 0 = K >= 256, else K / 32)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void gemm_rt_kernel(Planes A, const u16* __restrict__ Wf, int M, int N, int K,
                                                                                                 PlanesEpilogue pe, unsigned long long* __restrict__ clk) {
    const int KS = K >> 4, KT = K >> 5;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    M = pe.rows(M);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // optional phase clock (mi_debug_rt_clock): per workgroup [8] = s_memtime at entry / first k-tile in LDS / end of the main loop / exit,
    // s_memrealtime (100 MHz) at entry and exit
    int stamp_i = 0;
    auto stamp = [&]() {
        if (clk && tid == 0) clk[(size_t)blockIdx.x * 8 + stamp_i] = __builtin_amdgcn_s_memtime();
        ++stamp_i;
    };
    stamp();
    if (clk && tid == 0) clk[(size_t)blockIdx.x * 8 + 4] = __builtin_amdgcn_s_memrealtime();
    const int l31 = lane & 31, kg = lane >> 5;
    const int ncb = N >> 8;
    const int id = blockIdx.x, slot = id >> 3, cb = slot % ncb, tile = (slot / ncb) * 8 + (id & 7);
    const int row0 = tile * 128;
    if (row0 >= M) return;

    const __amdgpu_buffer_rsrc_t rsa = uniform_rsrc(A.base + A.tile(tile, 0), A.KT * 24576);
    const int voffa = (lane >> 2) * 64 + (((lane & 3) ^ ((lane >> 4) & 3)) << 4);
    auto dma_tile = [&](int kt, int st) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int piece = wave * 4 + q;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsa, (__attribute__((address_space(3))) void*)(smem + st * EG2B_STAGE + piece * 1024), 16, voffa,
                                                     kt * 24576 + (piece >> 3) * 8192 + (piece & 7) * 1024, 0, 0);
        }
    };
    dma_tile(0, 0);
    dma_tile(1, 1);
    dma_tile(2, 2);

    int voffw[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) voffw[t] = lane * 16 + ((8 * cb + 2 * wave + t) * KS) * 2048;
    u32x4 ring[4][2][2];
    // (inline asm, with a counted wait in front of every step's MFMAs: see MI_RING_WAIT)
    const u32x4 rsw_s = rsrc_words(Wf, N * K * 4);
    auto ring_load = [&](int ks, u32x4 (&w)[2][2]) {
        const int soff = __builtin_amdgcn_readfirstlane(ks * 2048);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(w[t][0]) : "v"(voffw[t]), "s"(rsw_s), "s"(soff));
            asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen offset:1024" : "=v"(w[t][1]) : "v"(voffw[t]), "s"(rsw_s), "s"(soff));
        }
    };
    // (inside the loop the slot is a read-write operand of its own reload: the slice stays in the registers the prologue gave it, from the
    //  first request to the last product -- no new value for the register allocator to place somewhere else)
    auto ring_reload = [&](int ks, u32x4 (&w)[2][2]) {
        const int soff = __builtin_amdgcn_readfirstlane(ks * 2048);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "+v"(w[t][0]) : "v"(voffw[t]), "s"(rsw_s), "s"(soff));
            asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen offset:1024" : "+v"(w[t][1]) : "v"(voffw[t]), "s"(rsw_s), "s"(soff));
        }
    };
#pragma unroll
    for (int d = 0; d < 4; ++d) ring_load(d, ring[d]);

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // (fragment reads as inline asm, as in edge_gemm2b_kernel)
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
    unsigned rd_off[2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) rd_off[s2] = lds0 + (unsigned)(l31 * 64 + (((2 * s2 + kg) ^ ((l31 >> 2) & 3)) * 16));
    auto read_a = [&](int st, int s2, f16x8 (&af)[4][2]) {
        const unsigned va = rd_off[s2] + (unsigned)st * EG2B_STAGE;
#define MI_RD128(dst, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(va), "n"(off))
        MI_RD128(af[0][0], 0 * 2048);        MI_RD128(af[0][1], 0 * 2048 + 8192);
        MI_RD128(af[1][0], 1 * 2048);        MI_RD128(af[1][1], 1 * 2048 + 8192);
        MI_RD128(af[2][0], 2 * 2048);        MI_RD128(af[2][1], 2 * 2048 + 8192);
        MI_RD128(af[3][0], 3 * 2048);        MI_RD128(af[3][1], 3 * 2048 + 8192);
#undef MI_RD128
    };
    auto mma = [&](const u32x4 (&w)[2][2], f16x8 (&af)[4][2]) {   // (two row blocks at a time, each pair behind the wait for its own fragments)
#pragma unroll
        for (int ip = 0; ip < 2; ++ip) {
            if (ip == 0) asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(af[0][0]), "+v"(af[0][1]), "+v"(af[1][0]), "+v"(af[1][1]));
            else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(af[2][0]), "+v"(af[2][1]), "+v"(af[3][0]), "+v"(af[3][1]));
#pragma unroll
            for (int term = MI_TERM0; term < 3; ++term)
#pragma unroll
                for (int i = 2 * ip; i < 2 * ip + 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        if constexpr (LEAN)   // operands swapped: the tile arrives transposed, a lane holds one output ROW (planes_epilogue_lean)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, w[j][term == 1 ? 1 : 0]), af[i][term == 0 ? 1 : 0], acc[i][j], 0, 0, 0);
                        else
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i][term == 0 ? 1 : 0], __builtin_bit_cast(f16x8, w[j][term == 1 ? 1 : 0]), acc[i][j], 0, 0, 0);
        }
    };
    // (waits as in edge_gemm2b_kernel, counted for any even KT: loop_waits.h.  EXT: touching the epilogue's row-wise operands 3 / 5 / 8 k-tiles
    //  before the loop ends measured no gain -- docs/rounds/round4.md 18.4; last present at 3e3d930)
    unsigned long long t_first = 0;
    auto head = [&](int k, auto hw, auto dma, auto mark) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(decltype(hw)::value) : "memory");
        MI_LOOP_BARRIER();
        if (decltype(mark)::value == LW_MARK_FIRST && clk) MI_LOOP_STAMP(t_first);
        if (decltype(dma)::value) dma_tile(k + 3, (k + 3) & 3);
    };
    auto step = [&](int k, auto slot, auto rw, auto issue) {
        constexpr int SL = decltype(slot)::value, s2 = SL & 1;
        f16x8 af[4][2];
        read_a(k & 3, s2, af);
        MI_RING_WAIT(ring[SL], decltype(rw)::value);
        mma(ring[SL], af);
        if (decltype(issue)::value) ring_reload(2 * k + s2 + 4, ring[SL]);
        __builtin_amdgcn_sched_barrier(0);
    };
    lw_k_loop<4, 4, 4, FORM>(KT, head, step);
    if (clk && tid == 0) clk[(size_t)blockIdx.x * 8 + 1] = t_first;
    stamp_i = 2;
    __syncthreads();   // every wave is done with the stages: they become the epilogue's per-wave patches
    stamp();
    if constexpr (LEAN) planes_epilogue_lean<4, 2>(pe, acc, tile, cb * 256 + wave * 64, M, lane);
    else planes_epilogue_rows<4, 2, EXT>(pe, acc, row0, cb * 256 + wave * 64, M, N, lane, reinterpret_cast<float*>(smem) + wave * 1152);
    stamp();
    if (clk && tid == 0) clk[(size_t)blockIdx.x * 8 + 5] = __builtin_amdgcn_s_memrealtime();
}

// plane set [N x K] -> fragment order (exact copy): one thread per (row, 8-k chunk)
__global__ void pack_frag_from_planes_kernel(Planes W, int N, int K, u16* __restrict__ dst) {
    const int KS = K / 16;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)N * (K / 8)) return;
    const int r = (int)(idx / (K / 8)), ch = (int)(idx % (K / 8));
    const int ct = r >> 5, l31 = r & 31, ks = ch >> 1, kg = ch & 1;
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
        *reinterpret_cast<u32x4*>(dst + ((((size_t)ct * KS + ks) * 2 + pl) * 64 + kg * 32 + l31) * 8) = *reinterpret_cast<const u32x4*>(W.base + W.elem(r, ch * 8, pl));
}

// ------------------------------------------------------------------------------------------------------------------------------------
// First edge GEMM, pair mode (see PlanesEpilogue: one operand row per unordered atom pair, the sine half of K into one accumulator set,
// the cosine half into another, both directed edges emitted by the epilogue), in the same form: 128 pairs x 128 columns per four-wave
// workgroup, a wave owns 128 pairs x 32 columns (4 x 1 MFMA tiles x two accumulator sets = 128 registers), the Fourier operand through
// four LDS stages by LDS-DMA, the weights in fragment order straight from L2 into a register ring, two workgroups per CU.  The plane
// GEMM's form of this product staged BOTH operands through registers into LDS (48 KiB of ds_write_b128 and 64 fragment reads per
// k-tile for 96 MFMAs): its main loop ran at 42 % of the matrix pipe's floor.  Epilogue, folded-in activation scales and self-edge
// workgroups are the plane GEMM's (planes_epilogue_pairs / act_scales_eval), so M1 is bit-identical to its output.
// ------------------------------------------------------------------------------------------------------------------------------------
int g_edge1_fused = 9;   // 9 = form b (edge_gemm1b_kernel) for launches beyond the plane GEMM's latency forms, 0 = the plane GEMM always, 1 .. 4 = form b whatever the size.
                         // (Round 3 measured form b equal to the plane GEMM, 191.8 vs 186.6 us at B = 256, and concluded "bound by its epilogue, not by its
                         //  loop"; its loop was being drained by compiler-inserted waits, and with those gone it is 3-6 % ahead end to end.)

// fragment-order pack of the Fourier block of edge_mlp.0 in the pair-mode column layout [sin block | pad | cos block | pad] (2 Kh columns)
__global__ void pack_frag_wff_pair_kernel(const float* __restrict__ W1, int edge_in, int H, int F, int Kh, u16* __restrict__ dst) {
    const int K = 2 * Kh, KS = K / 16, F3 = 3 * F;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // one (row, 8-k chunk) per thread
    if (idx >= (int64_t)H * (K / 8)) return;
    const int r = (int)(idx / (K / 8)), ch = (int)(idx % (K / 8));
    const int ct = r >> 5, l31 = r & 31, ks = ch >> 1, kg = ch & 1;
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = ch * 8 + i, blk = c >= Kh, cc = blk ? c - Kh : c;
        v[i] = cc < F3 ? W1[(size_t)r * edge_in + 2 * H + 9 + blk * F3 + cc] : 0.f;
    }
    u32x4 pk[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        unsigned p[3];
        pl_split_pair(v[2 * i], v[2 * i + 1], PL_SW, p);
        pk[0][i] = p[0];
        pk[1][i] = p[1];
    }
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) *reinterpret_cast<u32x4*>(dst + ((((size_t)ct * KS + ks) * 2 + pl) * 64 + kg * 32 + l31) * 8) = pk[pl];
}

// D: depth of the weight ring in k-steps (also in edge_gemm2b_kernel).  WIDE: the pair epilogue's 64-bit addressing, see PlanesEpilogue::pair_wide.
// A wave owns all 128 pairs of the tile and one 32-column MFMA tile: every activation fragment read from LDS feeds ONE column tile, 8 ds_read_b128
// per 12 MFMAs.  (A 128 x 256-tile form with 512 registers per lane and a 2 x 2-wave form of 64 x 64 measured 11-13 % slower, a one-accumulator-set
// form that multiplies the sine half twice no faster: docs/rounds/round3.md 16.3a, round4.md 18.4e; last present at 3e3d930.)
template <int D, bool WIDE, int FORM>   // FORM: the unrolled form of the k-loop (loop_waits.h lw_form: 0 = K >= 256, else K / 32)
__device__ __forceinline__ void edge_gemm1_body(const Planes& A, const u16* __restrict__ Wf, int M, int N, int K, PlanesEpilogue& pe, unsigned long long* clk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, kg = lane >> 5;
    constexpr int MI = 4, NJ = 1;   // 32-row x 32-column MFMA tiles per wave: a wave owns all 128 pairs of the tile and one column tile
    constexpr int WM = 4 / MI, WN = 4 / WM, WGC = 32 * NJ * WN;   // wave rows x wave columns of the workgroup, its columns
    const int KT = K / 32, KS = K / 16, nq = N / WGC;   // k-tiles, k-steps, column blocks of a row tile
    const int wm = wave / WN, wn = wave % WN;
    const int id = blockIdx.x;
    // this layer's M1 scale from the absmax slots and the weight bounds; workgroup 0 publishes all six scales (as the plane GEMM does) -- with
    // self edges in the launch that is the first self-edge workgroup, without them pair tile 0: edge_gemm2b_kernel and the node chain read them
    float cps_local = 0.f;
    auto eval_scales = [&]() {
        if (pe.sc_pq) {
            float dsc[6];
            act_scales_eval(__uint_as_float(pe.sc_pq[0]), __uint_as_float(pe.sc_gmax[0]), pe.sc_wb, dsc);
            cps_local = dsc[0];
            if (id == 0 && tid < 6) {
                pe.sc_dsc[tid] = dsc[tid];
                if (pe.sc_dsc2) pe.sc_dsc2[tid] = dsc[tid];
            }
        }
    };
    // ---- self edges (d = 0: the Fourier term is the constant C0): the FIRST pe.diag_blocks workgroups of the launch, eight nodes each ----
    // They take slots when the launch starts instead of queueing behind its pair tiles (behind them they were the launch's last arrivals, each
    // holding half a CU for a chain of dependent loads).  A thread owns one (node, 8-column chunk) item, two of them at H = 512, and requests
    // every load of both up front -- from clamped indices, masked at the use, as the pair epilogue's index loads are -- so that one memory
    // latency (two for G, whose row hangs on node2graph) covers the workgroup's life; a plane's eight halfs leave as ONE 16-byte store (eight
    // consecutive columns of a 32-column piece are contiguous in the tile-blocked layout).  Same sums in the same order as before:
    // v = C0 + ((P_i + P_j) + G), silu_fast, pl_split_pair.  They use no LDS (the launch's dynamic LDS is per launch: they hold it unused).
    if (id < pe.diag_blocks) {
        if (id * 8 >= pe.diag_nodes) return;   // (diag_blocks is rounded up to a multiple of 8: see the pair tiles' mapping below)
        const bool clocked = clk && tid == 0 && id < (int)gridDim.x - pe.diag_blocks;   // phase clock: entry / exit of self-edge workgroup d in slots 4 / 5 of row d
        if (clocked) clk[(size_t)id * 8 + 4] = __builtin_amdgcn_s_memtime();
        const int nch = N >> 3, items = 8 * nch;   // 8-column chunks of a node, items of the workgroup
        const float* PQ = pe.ep.row_bias;
        const int ldpq = pe.ep.ld_row_bias;
        for (int base = 0; base < items; base += 512) {
            bool ok[2];
            int col[2], e[2], g[2];
            f32x4 pi[2][2], pj[2][2], c0[2][2], gv[2][2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {   // index loads first: G's address waits for them alone
                const int item = base + tid + 256 * u, itc = item < items ? item : items - 1;
                const int node = id * 8 + itc / nch, nc = node < pe.diag_nodes ? node : pe.diag_nodes - 1;
                ok[u] = item < items && node < pe.diag_nodes;
                col[u] = (itc % nch) * 8;
                e[u] = pe.diag_e[nc];
                g[u] = pe.diag_node2graph[nc];
                const float* pr = PQ + (size_t)nc * ldpq + col[u];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    pi[u][h] = *reinterpret_cast<const f32x4*>(pr + 4 * h);
                    pj[u][h] = *reinterpret_cast<const f32x4*>(pr + N + 4 * h);
                    c0[u][h] = *reinterpret_cast<const f32x4*>(pe.diag_C0 + col[u] + 4 * h);
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const float* gr = pe.ep.row_bias3 + (size_t)g[u] * pe.ep.ld_row_bias3 + col[u];
#pragma unroll
                for (int h = 0; h < 2; ++h) gv[u][h] = *reinterpret_cast<const f32x4*>(gr + 4 * h);
            }
            if (base == 0) eval_scales();   // (its scalar loads and arithmetic run under the requests)
            const float cps = cps_local != 0.f ? cps_local : pe.Cp.s();
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (!ok[u]) continue;
                f32x4 v[2];
                u32x4 o[NPL];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) v[h][t] = c0[u][h][t] + ((pi[u][h][t] + pj[u][h][t]) + gv[u][h][t]);
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        unsigned p[3];
                        pl_split_pair(silu_fast(v[h][2 * t]), silu_fast(v[h][2 * t + 1]), cps, p);
#pragma unroll
                        for (int k = 0; k < NPL; ++k) o[k][2 * h + t] = p[k];
                    }
                }
                if (pe.ep.pre_act) {   // (training forward: the self edges' pre-activation is on the tape too)
                    float* z = pe.ep.pre_act + (size_t)e[u] * pe.ep.ld_pre + col[u];
                    *reinterpret_cast<f32x4*>(z) = v[0];
                    *reinterpret_cast<f32x4*>(z + 4) = v[1];
                }
#pragma unroll
                for (int k = 0; k < NPL; ++k) *reinterpret_cast<u32x4*>(pe.Cp.base + pe.Cp.elem(e[u], col[u], k)) = o[k];
            }
        }
        if (clocked) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the stores of thread 0's wave have left: the exit stamp closes the workgroup's memory work)
            clk[(size_t)id * 8 + 5] = __builtin_amdgcn_s_memtime();
        }
        return;
    }
    // (evaluated in front of the operand loads: behind them -- so that its four dependent scalar loads would run under the LDS-DMA latency --
    //  measured 2 k cycles SLOWER per workgroup, 4.9 k -> 6.9 k to the first barrier: profiles/r5_index_loads_ab.log)
    eval_scales();
    // XCD-aware mapping: the column quarters of a row tile run on the same XCD.  Workgroups go round-robin to the 8 XCDs by their launch id;
    // the self-edge workgroups in front are a multiple of 8, so the pair tiles' ids are shifted by whole rounds and id & 7 is still the XCD.
    const int pid = id - pe.diag_blocks;
    const int slot = pid >> 3, qt = slot % nq, tile = (slot / nq) * 8 + (pid & 7);
    const int row0 = tile * 128;
    if (row0 >= M) return;
    int stamp_i = 0;
    auto stamp = [&]() {
        if (clk && tid == 0) clk[(size_t)(tile * nq + qt) * 8 + stamp_i] = __builtin_amdgcn_s_memtime();
        ++stamp_i;
    };
    stamp();

    const __amdgpu_buffer_rsrc_t rsa = uniform_rsrc(A.base + A.tile(tile, 0), A.KT * 24576);
    const int voffa = (lane >> 2) * 64 + (((lane & 3) ^ ((lane >> 4) & 3)) << 4);
    auto dma_tile = [&](int kt, int st) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int piece = wave * 4 + q;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsa, (__attribute__((address_space(3))) void*)(smem + st * EG2B_STAGE + piece * 1024), 16, voffa,
                                                     kt * 24576 + (piece >> 3) * 8192 + (piece & 7) * 1024, 0, 0);   // (aux 2 = non-temporal measured no gain: DESIGN 19.7)
        }
    };
    dma_tile(0, 0);
    dma_tile(1, 1);
    dma_tile(2, 2);
    const __amdgpu_buffer_rsrc_t rsw = uniform_rsrc(Wf, N * K * 4);
    int voffw[NJ];   // the wave's column tiles: columns WGC qt + 32 NJ wn + 32 t .. + 31
#pragma unroll
    for (int t = 0; t < NJ; ++t) voffw[t] = lane * 16 + (((WN * qt + wn) * NJ + t) * KS) * 2048;
    u32x4 ring[D][NJ][2];
    // (every memory operation of the k-loop under manual control, as in edge_gemm2b_kernel -- a weight slice is two loads here, so 6 ring loads
    //  and 8 LDS-DMA pieces are issued behind one before its use: vmcnt(14))
    const u32x4 rsw_s = rsrc_words(Wf, N * K * 4);
    auto ring_load = [&](int ks, u32x4 (&w)[NJ][2]) {
        const int soff = __builtin_amdgcn_readfirstlane(ks * 2048);
        asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(w[0][0]) : "v"(voffw[0]), "s"(rsw_s), "s"(soff));
        asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen offset:1024" : "=v"(w[0][1]) : "v"(voffw[0]), "s"(rsw_s), "s"(soff));
    };
    auto ring_reload = [&](int ks, u32x4 (&w)[NJ][2]) {   // (read-write, as in edge_gemm2b_kernel: the slot keeps its registers)
        const int soff = __builtin_amdgcn_readfirstlane(ks * 2048);
        asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "+v"(w[0][0]) : "v"(voffw[0]), "s"(rsw_s), "s"(soff));
        asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen offset:1024" : "+v"(w[0][1]) : "v"(voffw[0]), "s"(rsw_s), "s"(soff));
    };
#pragma unroll
    for (int d = 0; d < D; ++d) ring_load(d, ring[d]);

    f32x16 acc[MI][NJ], accS[MI][NJ];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
    unsigned rd_off[2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) rd_off[s2] = lds0 + (unsigned)(l31 * 64 + (((2 * s2 + kg) ^ ((l31 >> 2) & 3)) * 16));
    auto read_a = [&](int st, int s2, f16x8 (&af)[MI][2]) {
        const unsigned va = rd_off[s2] + (unsigned)st * EG2B_STAGE;
#define MI_RD128(dst, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(va), "n"(off))
        MI_RD128(af[0][0], 0 * 2048);        MI_RD128(af[0][1], 0 * 2048 + 8192);
        MI_RD128(af[1][0], 1 * 2048);        MI_RD128(af[1][1], 1 * 2048 + 8192);
        MI_RD128(af[2][0], 2 * 2048);        MI_RD128(af[2][1], 2 * 2048 + 8192);
        MI_RD128(af[3][0], 3 * 2048);        MI_RD128(af[3][1], 3 * 2048 + 8192);
#undef MI_RD128
    };
    auto mma = [&](u32x4 (&w)[NJ][2], f16x8 (&af)[MI][2], auto rw) {   // terms (a1, b0), (a0, b1), (a0, b0); the slice has landed at vmcnt(rw)
        asm volatile("s_waitcnt vmcnt(%2)" : "+v"(w[0][0]), "+v"(w[0][1]) : "n"(decltype(rw)::value));
#pragma unroll
        for (int ip = 0; ip < 2; ++ip) {   // two row blocks at a time, each pair behind the wait for its own fragments
            if (ip == 0) asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(af[0][0]), "+v"(af[0][1]), "+v"(af[1][0]), "+v"(af[1][1]));
            else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(af[2][0]), "+v"(af[2][1]), "+v"(af[3][0]), "+v"(af[3][1]));
#pragma unroll
            for (int term = MI_TERM0; term < 3; ++term)
#pragma unroll
                for (int i = 2 * ip; i < 2 * ip + 2; ++i)
                    acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i][term == 0 ? 1 : 0], __builtin_bit_cast(f16x8, w[0][term == 1 ? 1 : 0]), acc[i][0], 0, 0, 0);
        }
    };
    static_assert(D == 4, "two k-tiles of ring per unrolled pair of iterations");
    const int khalf = KT / 2;
    // Every wait of the loop is counted, from the fill to the drain (loop_waits.h: per k-tile this wave issues 4 DMA pieces and then 2 x 2 ring loads;
    // vector memory operations retire in order, so a k-tile or a slice has landed once no more operations are outstanding than were issued behind
    // it).  The phase clock keeps its two in-loop stamps in scalar registers and stores them behind the loop (MI_LOOP_STAMP).
    unsigned long long t_first = 0, t_tail = 0;
    auto head = [&](int k, auto hw, auto dma, auto mark) {
        if (k == khalf) {   // the cosine half of K goes into the second accumulator set
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    accS[i][j] = acc[i][j];
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
                }
        }
        if (decltype(mark)::value == LW_MARK_TAIL && clk) MI_LOOP_STAMP(t_tail);   // head of the third iteration from the end
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(decltype(hw)::value) : "memory");
        MI_LOOP_BARRIER();
        if (decltype(mark)::value == LW_MARK_FIRST && clk) MI_LOOP_STAMP(t_first);
        if (decltype(dma)::value) dma_tile(k + 3, (k + 3) & 3);
    };
    auto step = [&](int k, auto slot, auto rw, auto issue) {
        constexpr int SL = decltype(slot)::value, s2 = SL & 1;
        f16x8 af[MI][2];
        read_a(k & 3, s2, af);
        mma(ring[SL], af, rw);
        if (decltype(issue)::value) ring_reload(2 * k + s2 + D, ring[SL]);
        __builtin_amdgcn_sched_barrier(0);
    };
    lw_k_loop<4, 2 * NJ, D, FORM>(KT, head, step);
    stamp_i = 2;
    stamp();
    if (clk && tid == 0) {
        clk[(size_t)(tile * nq + qt) * 8 + 1] = t_first;
        clk[(size_t)(tile * nq + qt) * 8 + 6] = t_tail;
    }
    __syncthreads();   // the epilogue's per-wave patches overlay the operand stages
    planes_epilogue_pairs<MI, NJ, WIDE>(pe, accS, acc, row0 + wm * MI * 32, qt * WGC + wn * 32 * NJ, M, N, lane, reinterpret_cast<float*>(smem) + wave * 2304, cps_local);
    stamp();
}

template <int D, bool WIDE, int FORM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void edge_gemm1b_kernel(Planes A, const u16* __restrict__ Wf, int M, int N, int K,
                                                                                                     PlanesEpilogue pe, unsigned long long* clk) {
    edge_gemm1_body<D, WIDE, FORM>(A, Wf, M, N, K, pe, clk);
}

unsigned long long* g_edge1_clk = nullptr;

// (timing experiment, mi_debug_set_skip bit 5: an EMPTY launch in front of every edge GEMM -- 24 more kernel boundaries per step on a chain's serial path and no
//  work: what a boundary costs the four-chain step, i.e. what removing launches from the path can buy: DESIGN 19.9)
__global__ void empty_boundary_kernel() {}

int edge_gemm1(mi_net* net, const Planes& A, int layer, int M, PlanesEpilogue pe, hipStream_t s) {
    if (g_ablate_skip & 2) return MI_OK;
    if (g_ablate_skip & 32) hipLaunchKernelGGL(empty_boundary_kernel, dim3(1), dim3(64), 0, s);
    static std::once_flag once;
    static hipError_t attr_err = hipSuccess;
    std::call_once(once, [] {
        auto set = [](auto form) {
            constexpr int F = decltype(form)::value;
            if (attr_err == hipSuccess) attr_err = hipFuncSetAttribute((const void*)edge_gemm1b_kernel<4, true, F>, hipFuncAttributeMaxDynamicSharedMemorySize, EG2B_LDS);
            if (attr_err == hipSuccess) attr_err = hipFuncSetAttribute((const void*)edge_gemm1b_kernel<4, false, F>, hipFuncAttributeMaxDynamicSharedMemorySize, EG2B_LDS);
        };
        set(LwInt<0>{});
        set(LwInt<2>{});
        set(LwInt<4>{});
        set(LwInt<6>{});
    });
    MI_HIP(attr_err);
    const int H = net->H, K = 2 * net->Kh;
    count_mfma(M, H, K, MI_PLANES_TERMS);   // (pair rows x [sine block | cosine block] of the Fourier columns)
    pe.out_scale = 1.f / (A.scale * PL_SW);
    int nblk = (H / 128) * ((cdiv(M, 128) + 7) / 8 * 8);
    if (pe.diag_C0) {   // the self-edge workgroups come first (a multiple of 8: the pair tiles keep their XCDs)
        pe.diag_blocks = (cdiv(pe.diag_nodes, 8) + 7) / 8 * 8;
        nblk += pe.diag_blocks;
    }
    const u16* Wf = net->Wffc + (size_t)layer * ((size_t)H * K * 2);
    lw_dispatch_form(K / 32, [&](auto form) {   // (one kernel instance per unrolled form of the k-loop: loop_waits.h)
        constexpr int F = decltype(form)::value;
        if (pe.pair_wide) hipLaunchKernelGGL((edge_gemm1b_kernel<4, true, F>), dim3(nblk), dim3(256), EG2B_LDS, s, A, Wf, M, H, K, pe, g_edge1_clk);
        else hipLaunchKernelGGL((edge_gemm1b_kernel<4, false, F>), dim3(nblk), dim3(256), EG2B_LDS, s, A, Wf, M, H, K, pe, g_edge1_clk);
        return 0;
    });
    MI_KERNEL_CHECK();
    return MI_OK;
}

// whether layer launches of M pair rows take edge_gemm1: forced (1 .. 4: tests) whatever the size; by default (9) for the
// launches beyond the plane GEMM's latency forms -- with its k-loop under manual control it beats the plane GEMM there
bool edge_gemm1_supported(const mi_net* net, int64_t M) {
    if (!(net->H % 128 == 0 && net->Wffc != nullptr && (2 * net->Kh) % 64 == 0) || g_edge1_fused == 0) return false;
    if (g_edge1_fused != 9) return true;
    return (int64_t)(net->H / 128) * ((cdiv(M, 128) + 7) / 8 * 8) > g_planes_lat_max_blocks;
}

int edge_gemm1_pack(mi_net* net, int l, const float* W1, hipStream_t s) {
    const int H = net->H, K = 2 * net->Kh;
    hipLaunchKernelGGL(pack_frag_wff_pair_kernel, dim3(cdiv((int64_t)H * (K / 8), 256)), dim3(256), 0, s, W1, net->edge_in, H, net->F, net->Kh,
                       net->Wffc + (size_t)l * ((size_t)H * K * 2));
    MI_KERNEL_CHECK();
    return MI_OK;
}

unsigned long long* g_edge2_clk = nullptr;

int edge_gemm2(mi_net* net, mi_batch* b, int layer, hipStream_t s, float* Z2) {
    if (g_ablate_skip & 4) return MI_OK;
    if (g_ablate_skip & 32) hipLaunchKernelGGL(empty_boundary_kernel, dim3(1), dim3(64), 0, s);
    static std::once_flag once;
    static hipError_t attr_err = hipSuccess;
    std::call_once(once, [] {
        attr_err = hipFuncSetAttribute((const void*)edge_gemm2b_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, EG2B_LDS);
        if (attr_err == hipSuccess) attr_err = hipFuncSetAttribute((const void*)edge_gemm2b_kernel<4, true>, hipFuncAttributeMaxDynamicSharedMemorySize, EG2B_LDS);
    });
    MI_HIP(attr_err);
    const int H = net->H;
    count_mfma(b->E, H, H, MI_PLANES_TERMS);
    EdgeGemm2Args a;
    a.A = make_planes(b->m1_cur ? b->m1_cur : b->M1pl, H, PL_S_ACT, b->dsc);
    a.W2f = net->Wnc + (size_t)layer * node_chain_pack_elems(H) + (size_t)5 * H * H * 2;
    a.b2 = net->p("csp_layer_" + std::to_string(layer) + ".edge_mlp.2.bias");
    a.dsc = b->dsc;
    a.src = b->src;
    a.rowptr = b->rowptr;
    a.part = b->part;
    a.E = (int)b->E;
    a.N = b->N;
    {   // the per-tile tables of this graph (fc: built once per batch handle; knn: the forward that rebuilt the edge list bumped graph_epoch)
        const int tiles_cap = cdiv(b->E_cap, 128);
        if (!b->e2_tab) MI_TRY(dev_alloc(b, &b->e2_tab, (size_t)tiles_cap * EG2_TAB));
        if (b->e2_tab_epoch != b->graph_epoch) {
            hipLaunchKernelGGL(edge2_tables_kernel, dim3(cdiv(b->E, 128)), dim3(128), 0, s, b->src, b->rowptr, (int)b->E, b->N, b->e2_tab);
            MI_KERNEL_CHECK();
            b->e2_tab_epoch = b->graph_epoch;
        }
        a.tab = b->e2_tab;
    }
    a.Z2 = Z2;
    a.clk = g_edge2_clk;
    if (Z2) {   // the training forward: form B with the pre-activation kept (written row-major through per-wave LDS patches)
        hipLaunchKernelGGL((edge_gemm2b_kernel<4, true>), dim3(2 * ((cdiv(b->E, 128) + 7) / 8 * 8)), dim3(256), EG2B_LDS, s, a);
        MI_KERNEL_CHECK();
        return MI_OK;
    }
    // form B -- 128 x 256 tiles, four waves, two workgroups per CU (any non-zero g_edge2_fused)
    hipLaunchKernelGGL((edge_gemm2b_kernel<4>), dim3(2 * ((cdiv(b->E, 128) + 7) / 8 * 8)), dim3(256), EG2B_LDS, s, a);
    MI_KERNEL_CHECK();
    return MI_OK;
}

bool edge_gemm2_supported(const mi_net* net) { return g_edge2_fused && net->H == 512 && net->Wnc != nullptr; }

unsigned long long* g_rt_clk = nullptr;   // phase clock of gemm_rt launches (mi_debug_rt_clock): [workgroup][8]
int g_rt_clk_ext = -1;                    // -1: every launch writes it (the last one stays); 0 / 1: launches of the plain / the extended epilogue only
int g_rt_lean = 1;                        // the lean epilogue for the launches that qualify (planes_epilogue_is_lean); 0: the general one for all
int g_rt_clk_skip = 0;                    // matching launches to let pass before the one that is clocked (then the clock switches itself off)

int gemm_rt(const Planes& A, const u16* Wfrag, int M, int N, int K, const PlanesEpilogue& pe, bool ext, hipStream_t s) {
    static std::once_flag once;
    static hipError_t attr_err = hipSuccess;
    std::call_once(once, [] {
        auto set = [](auto form) {
            constexpr int F = decltype(form)::value;
            if (attr_err == hipSuccess) attr_err = hipFuncSetAttribute((const void*)gemm_rt_kernel<false, false, F>, hipFuncAttributeMaxDynamicSharedMemorySize, EG2B_NST * EG2B_STAGE);
            if (attr_err == hipSuccess) attr_err = hipFuncSetAttribute((const void*)gemm_rt_kernel<true, false, F>, hipFuncAttributeMaxDynamicSharedMemorySize, EG2B_NST * EG2B_STAGE);
            if (attr_err == hipSuccess) attr_err = hipFuncSetAttribute((const void*)gemm_rt_kernel<false, true, F>, hipFuncAttributeMaxDynamicSharedMemorySize, EG2B_NST * EG2B_STAGE);
        };
        set(LwInt<0>{});
        set(LwInt<2>{});
        set(LwInt<4>{});
        set(LwInt<6>{});
        if (const char* e = getenv("MI_RT_LEAN")) g_rt_lean = atoi(e) & 3;   // (A/B runs of whole test files: scripts/gpu_rt_lean_ab.sh; 2 behaves as 1)
    });
    MI_HIP(attr_err);
    MI_CHECK(Wfrag && (N & 255) == 0 && (K & 63) == 0 && K >= 64 && A.KT >= K / 32, MI_EINVAL, "gemm_rt: N % 256, K % 64, K >= 64 and a fragment-order W operand");
    if (M <= 0) return MI_OK;
    count_mfma(M, N, K, MI_PLANES_TERMS);
    const dim3 grid((N >> 8) * ((cdiv(M, 128) + 7) / 8 * 8));
    static const bool trace = getenv("MI_RT_TRACE") != nullptr;   // (debugging aid: which epilogue features each launch carries)
    if (trace)
        fprintf(stderr, "gemm_rt M=%d N=%d K=%d ext=%d act=%d bias=%d rb=%d%d%d pre_add=%d pre_act=%d res=%d res_pl=%d os=%g res2=%d res2_pl=%d rows2=%d post_mul=%d C=%d Cp=%d absmax=%d\n", M, N, K,
                (int)ext, pe.ep.act, !!pe.ep.bias, !!pe.ep.row_bias, !!pe.ep.row_bias2, !!pe.ep.row_bias3, !!pe.ep.pre_add, !!pe.ep.pre_act, !!pe.ep.residual, !!pe.res_pl.base,
                (double)pe.ep.out_scale, !!pe.residual2, !!pe.res2_pl.base, !!pe.res2_rows, !!pe.post_mul, !!pe.C, !!pe.Cp.base, !!pe.absmax);
    unsigned long long* clk = nullptr;
    if (g_rt_clk && (g_rt_clk_ext < 0 || g_rt_clk_ext == (int)ext)) {
        if (g_rt_clk_skip > 0) {
            --g_rt_clk_skip;
        } else {
            clk = g_rt_clk;
            if (g_rt_clk_ext >= 0) g_rt_clk = nullptr;   // one launch
        }
    }
    lw_dispatch_form(K / 32, [&](auto form) {   // (one kernel instance per unrolled form of the k-loop: loop_waits.h)
        constexpr int F = decltype(form)::value;
        if (g_rt_lean && planes_epilogue_is_lean(pe)) hipLaunchKernelGGL((gemm_rt_kernel<false, true, F>), grid, dim3(256), EG2B_NST * EG2B_STAGE, s, A, Wfrag, M, N, K, pe, clk);
        else if (ext) hipLaunchKernelGGL((gemm_rt_kernel<true, false, F>), grid, dim3(256), EG2B_NST * EG2B_STAGE, s, A, Wfrag, M, N, K, pe, clk);
        else hipLaunchKernelGGL((gemm_rt_kernel<false, false, F>), grid, dim3(256), EG2B_NST * EG2B_STAGE, s, A, Wfrag, M, N, K, pe, clk);
        return 0;
    });
    MI_KERNEL_CHECK();
    return MI_OK;
}

size_t frag_elems(int N, int K) { return (size_t)N * K * 2; }

int pack_frag_from_planes(const Planes& W, int N, int K, u16* dst, hipStream_t s) {
    MI_CHECK((N & 31) == 0 && (K & 15) == 0, MI_EINVAL, "pack_frag_from_planes: N % 32, K % 16");
    hipLaunchKernelGGL(pack_frag_from_planes_kernel, dim3((unsigned)cdiv((int64_t)N * (K / 8), 256)), dim3(256), 0, s, W, N, K, dst);
    MI_KERNEL_CHECK();
    return MI_OK;
}

#else

int gemm_rt(const Planes&, const u16*, int, int, int, const PlanesEpilogue&, bool, hipStream_t) { return MI_ESTATE; }
size_t frag_elems(int N, int K) { return (size_t)N * K * 2; }
int pack_frag_from_planes(const Planes&, int, int, u16*, hipStream_t) { return MI_ESTATE; }

int edge_gemm2(mi_net*, mi_batch*, int, hipStream_t, float*) { return MI_ESTATE; }
bool edge_gemm2_supported(const mi_net*) { return false; }
int edge_gemm1(mi_net*, const Planes&, int, int, PlanesEpilogue, hipStream_t) { return MI_ESTATE; }
bool edge_gemm1_supported(const mi_net*, int64_t) { return false; }
int edge_gemm1_pack(mi_net*, int, const float*, hipStream_t) { return MI_OK; }
int g_edge1_fused = 0;

#endif

}  // namespace mi

extern "C" int mi_debug_set_rt_lean(int on) {
#if MI_PLANES_FP16
    const int was = mi::g_rt_lean;
    mi::g_rt_lean = on & 3;   // (2 behaves as 1; the bits above are ignored: they sized a persistent grid that is gone)
    return was;
#else
    (void)on;
    return 0;
#endif
}

extern "C" int mi_debug_rt_clock(void* dev_buffer, int ext, int skip) {
#if MI_PLANES_FP16
    mi::g_rt_clk = (unsigned long long*)dev_buffer;
    mi::g_rt_clk_ext = ext;
    mi::g_rt_clk_skip = skip;
#else
    (void)dev_buffer; (void)ext; (void)skip;
#endif
    return MI_OK;
}

extern "C" int mi_debug_edge2_clock(void* dev_buffer) {
#if MI_PLANES_FP16
    mi::g_edge2_clk = (unsigned long long*)dev_buffer;
#endif
    return MI_OK;
}

extern "C" int mi_debug_edge1_clock(void* dev_buffer) {
#if MI_PLANES_FP16
    mi::g_edge1_clk = (unsigned long long*)dev_buffer;
#endif
    return MI_OK;
}

extern "C" int mi_debug_set_edge2_fused(int on) {
    // (returns the previous MODE, so that save-and-restore through the return value is exact: 4 = inference forwards only)
    const int was = (mi::g_edge2_fused == 1 && !mi::g_edge2_train) ? 4 : mi::g_edge2_fused;
    mi::g_edge2_fused = on == 4 ? 1 : on;
    mi::g_edge2_train = on == 1;   // (4: inference forwards only -- the training forward keeps the 128 x 128 plane GEMM)
    return was;
}

extern "C" int mi_debug_set_edge_fused(int) { return 0; }   // (retired: the one-launch edge stage is gone, the setting was and stays off)

extern "C" int mi_debug_set_edge1_fused(int on) {
    const int was = mi::g_edge1_fused;
    mi::g_edge1_fused = on;
    return was;
}
