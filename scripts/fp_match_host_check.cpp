// The fingerprint-matching kernels' own source (matinvent_amd/csrc/fp_match_body.h) run on the host: blockIdx and threadIdx are loop
// variables, a barrier is the end of a phase's thread loop, a lane exchange of the butterfly goes through an array of the 64 lanes' values.
// Every array is allocated at exactly its size (the LDS tile at the size the launch would give it), so that the host sanitizers see any
// index past an end -- also for a candidate list with out-of-range and wrong-length entries, which the guard must skip without a read:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/fp_match_host_check.cpp -o fp_match_host_check
//   ./fp_match_host_check case.bin out.bin
//
// case.bin (little endian, written by tests/test_fp_match_host.py): int32 Q, row_stride, M, G, nnz_q, nnz_c, pairs, chunk; int64
// bank_floats; float32 tol; then query [Q][row_stride], bank [bank_floats] as float32; bank_start [M] int64; bank_len [M], grp_q_off
// [G + 1], q_idx [nnz_q], grp_c_off [G + 1], c_idx [nnz_c], grp_ncols [G] as int32.  out.bin receives best_dist [Q] float32, best_idx,
// n_within, status [Q] int32 and, with pairs, the groups' pair matrices one after another (nan where a candidate was skipped), for a
// comparison with tests/fp_match_ref.py.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <vector>

#include "../matinvent_amd/csrc/fp_match_body.h"

using namespace mi;

template <class T>
static std::unique_ptr<T[]> read_array(FILE* f, size_t n) {
    std::unique_ptr<T[]> p(new T[n]);
    if (n && std::fread(p.get(), sizeof(T), n, f) != n) {
        std::fprintf(stderr, "case file cut short\n");
        std::exit(2);
    }
    return p;
}

static void level(FpmLane* regs, int wave, int mask, int half) {
    const int n = half ? half : 1;
    std::vector<float> send((size_t)FPM_WAVE * n);
    for (int lane = 0; lane < FPM_WAVE; ++lane) fpm_level_send(regs[wave * FPM_WAVE + lane], lane, mask, half, &send[(size_t)lane * n]);
    for (int lane = 0; lane < FPM_WAVE; ++lane) fpm_level_add(regs[wave * FPM_WAVE + lane], lane, mask, half, &send[(size_t)(lane ^ mask) * n]);
}

int main(int argc, char** argv) {
    if (argc < 3) return std::fprintf(stderr, "usage: %s case.bin out.bin\n", argv[0]), 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return std::perror(argv[1]), 2;
    int h[8];
    int64_t bank_floats;
    float tol;
    if (std::fread(h, sizeof(int), 8, f) != 8 || std::fread(&bank_floats, 8, 1, f) != 1 || std::fread(&tol, 4, 1, f) != 1) return 2;
    const int Q = h[0], stride = h[1], M = h[2], G = h[3], nnz_q = h[4], nnz_c = h[5], pairs = h[6], chunk = h[7];
    if (Q < 0 || stride < 0 || stride % 4 || M < 0 || G < 0 || nnz_q < 0 || nnz_c < 0 || bank_floats < 0) return std::fprintf(stderr, "bad header\n"), 2;
    auto query = read_array<float>(f, (size_t)Q * stride);
    auto bank = read_array<float>(f, (size_t)bank_floats);
    auto bank_start = read_array<int64_t>(f, M);
    auto bank_len = read_array<int>(f, M);
    auto q_off = read_array<int>(f, G + 1);
    auto q_idx = read_array<int>(f, nnz_q);
    auto c_off = read_array<int>(f, G + 1);
    auto c_idx = read_array<int>(f, nnz_c);
    auto ncols = read_array<int>(f, G);
    std::fclose(f);

    int64_t n_items = 0, n_parts = 0;
    int used = fpm_plan(q_off.get(), c_off.get(), G, chunk, nullptr, nullptr, &n_items, &n_parts);
    if (used <= 0) return std::fprintf(stderr, "plan refused the offsets\n"), 2;
    std::unique_ptr<int[]> items(new int[(size_t)n_items * MI_FP_MATCH_ITEM_INTS]), part_off(new int[G + 1]);
    used = fpm_plan(q_off.get(), c_off.get(), G, used, items.get(), part_off.get(), &n_items, &n_parts);
    std::unique_ptr<int64_t[]> pair_off(new int64_t[G]);
    int64_t pair_floats = 0;
    int max_ncols = 1;
    for (int g = 0; g < G; ++g) {
        pair_off[g] = pair_floats;
        pair_floats += (int64_t)(q_off[g + 1] - q_off[g]) * (c_off[g + 1] - c_off[g]);
        if (ncols[g] > max_ncols && ncols[g] <= FPM_MAX_LEN) max_ncols = ncols[g];
    }
    if (!pairs) pair_floats = 0;
    std::unique_ptr<float[]> best_dist(new float[Q]), pair_dist(new float[(size_t)pair_floats]), part_dist(new float[(size_t)n_parts]);
    std::unique_ptr<int[]> best_idx(new int[Q]), n_within(new int[Q]), status(new int[Q]);
    std::unique_ptr<int[]> part_idx(new int[(size_t)n_parts]), part_cnt(new int[(size_t)n_parts]), part_status(new int[(size_t)n_parts]);
    for (int q = 0; q < Q; ++q) best_dist[q] = std::numeric_limits<float>::infinity(), best_idx[q] = -1, n_within[q] = status[q] = 0;
    for (int64_t e = 0; e < n_parts; ++e) part_status[e] = FPM_UNWRITTEN;   // what the entry's fill does on the device
    for (int64_t e = 0; e < pair_floats; ++e) pair_dist[e] = std::numeric_limits<float>::quiet_NaN();

    FpmArgs A{};
    mi_fp_match_args& a = A.a;
    a.query = query.get(), a.bank = bank.get(), a.bank_start = bank_start.get(), a.bank_len = bank_len.get();
    a.grp_q_off = q_off.get(), a.q_idx = q_idx.get(), a.grp_c_off = c_off.get(), a.c_idx = c_idx.get(), a.grp_ncols = ncols.get();
    a.items = items.get(), a.grp_part_off = part_off.get(), a.workspace = nullptr;
    a.best_dist = best_dist.get(), a.best_idx = best_idx.get(), a.n_within = n_within.get(), a.status = status.get();
    a.pair_dist = pairs ? pair_dist.get() : nullptr, a.pair_off = pairs ? pair_off.get() : nullptr;
    a.bank_floats = bank_floats, a.pair_floats = pair_floats;
    a.Q = Q, a.row_stride = stride, a.M = M, a.G = G, a.nnz_q = nnz_q, a.nnz_c = nnz_c, a.n_items = (int)n_items, a.n_partials = (int)n_parts;
    a.max_ncols = max_ncols, a.tol = tol;
    A.part_dist = part_dist.get(), A.part_idx = part_idx.get(), A.part_cnt = part_cnt.get(), A.part_status = part_status.get();

    std::unique_ptr<float[]> tile(new float[(size_t)FPM_TQ * fpm_round4(max_ncols)]);   // the launch's dynamic LDS
    std::unique_ptr<FpmShared> s(new FpmShared);
    std::unique_ptr<FpmLane[]> regs(new FpmLane[FPM_THREADS]);
    const int masks[6] = {32, 16, 8, 4, 2, 1}, halves[6] = {16, 8, 4, 2, 1, 0};
    for (int item = 0; item < (int)n_items; ++item) {
        for (int tid = 0; tid < FPM_THREADS; ++tid) fpm_phase_item(*s, A, item, tid);
        for (int tid = 0; tid < FPM_THREADS; ++tid) fpm_phase_stage(*s, A, tile.get(), tid);
        if (!s->ok) continue;
        for (int tid = 0; tid < FPM_THREADS; ++tid) fpm_lane_init(regs[tid]);
        const int passes = (s->c1 - s->c0 + FPM_PASS - 1) / FPM_PASS;
        for (int pass = 0; pass < passes; ++pass) {
            for (int tid = 0; tid < FPM_THREADS; ++tid) fpm_pass_accumulate(*s, A, tile.get(), tid, pass, regs[tid]);
            for (int w = 0; w < FPM_WAVES; ++w)
                for (int l = 0; l < 6; ++l) level(regs.get(), w, masks[l], halves[l]);
            for (int tid = 0; tid < FPM_THREADS; ++tid) fpm_pass_update(*s, A, tid, pass, regs[tid]);
        }
        for (int tid = 0; tid < FPM_THREADS; ++tid) fpm_phase_wave_out(*s, tid, regs[tid]);
        for (int tid = 0; tid < FPM_THREADS; ++tid) fpm_phase_wave_status(*s, tid, regs[tid]);
        for (int tid = 0; tid < FPM_THREADS; ++tid) fpm_phase_partial(*s, A, tid);
    }
    const int blocks = (nnz_q + FPM_THREADS - 1) / FPM_THREADS;
    for (int p = 0; p < blocks * FPM_THREADS; ++p) fpm_reduce_query(A, p);

    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return std::perror(argv[2]), 2;
    std::fwrite(best_dist.get(), 4, Q, o);
    std::fwrite(best_idx.get(), 4, Q, o);
    std::fwrite(n_within.get(), 4, Q, o);
    std::fwrite(status.get(), 4, Q, o);
    std::fwrite(pair_dist.get(), 4, (size_t)pair_floats, o);
    std::fclose(o);
    std::printf("%d groups, %lld items of up to %d candidates, %lld partials, Q = %d, M = %d\n", G, (long long)n_items, used, (long long)n_parts, Q, M);
    return 0;
}
