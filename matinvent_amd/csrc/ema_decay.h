// The decay of the exponential moving average of the weights at applied step s (include/matinvent_hip_ema.h).  Host and
// device: the unguarded step forms it on the host, the guarded step forms it in every wave from the state block's adam_steps, and
// scripts/ema_host_check.cpp prints it; all three compile this text.
//
//   d_s = ema_warmup ? min(ema_decay, (1 + s) / (10 + s)) : ema_decay
//
// in float64, rounded to float once.  ema_decay is a float in [0, 1) (the entry refuses anything else), so the result is one too.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MI_EMA_HD __host__ __device__
#else
#define MI_EMA_HD
#endif

namespace mi {

MI_EMA_HD inline float ema_decay_at(float ema_decay, int ema_warmup, unsigned s) {
    if (!ema_warmup) return ema_decay;
    const double d = (double)ema_decay, w = (1.0 + (double)s) / (10.0 + (double)s);
    return (float)(d < w ? d : w);
}

}  // namespace mi
