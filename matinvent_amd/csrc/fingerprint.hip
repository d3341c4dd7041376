// Structure fingerprints (include/matinvent_hip_fp.h): one 256-thread block per crystal in the shape of structure_check_kernel,
// the species-resolved Oganov-Valle histogram in LDS as 64-bit fixed point (integer additions commute: bit-reproducible whatever the
// batch), normalised to a unit row.  The body lives in fingerprint_body.h, phase by phase, so that the host can run the same source.
#include "fingerprint_body.h"
#include "net.h"

namespace mi {

__global__ __launch_bounds__(FP_THREADS) void structure_fingerprint_kernel(FpArgs a) {
    __shared__ FpShared s;
    const int b = blockIdx.x, tid = threadIdx.x;
    fp_phase_init(s, a, b, tid);
    __syncthreads();
    fp_phase_scan(s, a, b, tid);
    __syncthreads();
    fp_phase_verdict(s, a, b, tid);
    __syncthreads();
    fp_phase_accumulate(s, a, b, tid);
    __syncthreads();
    fp_phase_weigh(s, a, b, tid);
    __syncthreads();
    fp_phase_norm(s, a, b, tid);
    __syncthreads();
    fp_phase_store(s, a, b, tid);
}

static int fingerprint_launch(const int* node_off, int B, const int* atom_types, const float* frac, const float* lattices,
                              const mi_fp_params* p, float* out_fp, float* out_info, hipStream_t stream) {
    MI_CHECK(node_off && atom_types && frac && lattices && p && out_fp && out_info && B >= 0, MI_EINVAL, "structure fingerprint: bad argument");
    MI_CHECK(p->r_max > 0.f && std::isfinite(p->r_max) && p->sigma > 0.f && std::isfinite(p->sigma), MI_EINVAL,
             "structure fingerprint: r_max = %g and sigma = %g must be positive and finite", (double)p->r_max, (double)p->sigma);
    MI_CHECK(p->nbins >= 1 && p->nbins <= MI_FP_MAX_BINS, MI_EINVAL, "structure fingerprint: nbins = %d outside 1..%d", p->nbins, MI_FP_MAX_BINS);
    if (B == 0) return MI_OK;
    FpArgs a;
    a.node_off = node_off;
    a.atom_types = atom_types;
    a.frac = frac;
    a.lattices = lattices;
    a.out_fp = out_fp;
    a.out_info = out_info;
    a.r_max = p->r_max;
    a.sigma = p->sigma;
    a.nbins = p->nbins;
    hipLaunchKernelGGL(structure_fingerprint_kernel, dim3(B), dim3(FP_THREADS), 0, stream, a);
    MI_KERNEL_CHECK();
    return MI_OK;
}

}  // namespace mi

using namespace mi;

extern "C" {

int mi_structure_fingerprint_offsets(const int* node_off, int B, const int* atom_types, const float* frac, const float* lattices,
                                     const mi_fp_params* params, float* out_fp, float* out_info, void* stream) {
    return fingerprint_launch(node_off, B, atom_types, frac, lattices, params, out_fp, out_info, (hipStream_t)stream);
}

int mi_structure_fingerprint(const mi_batch* b, const int* atom_types, const float* frac, const float* lattices, const mi_fp_params* params,
                             float* out_fp, float* out_info, void* stream) {
    MI_NO_POOLED(b, "mi_structure_fingerprint");
    MI_CHECK(b, MI_EINVAL, "structure fingerprint: null handle");
    return fingerprint_launch(b->node_off, b->B, atom_types, frac, lattices, params, out_fp, out_info, (hipStream_t)stream);
}

}  // extern "C"
