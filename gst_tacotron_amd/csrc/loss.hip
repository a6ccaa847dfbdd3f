// Validation losses of a teacher-forced pass: the four terms of the reference's Train_Step (Model.py:210-241) per utterance, as sums
// that the host reduces (gst_tacotron_amd/evaluate.py).  One kernel beside the decode step's own, off the mel-frame hot path.
//
//   gt_losses_kernel   one workgroup of 16 waves per utterance.  A prediction frame t and its target teacher[b, 1 + t] are both
//                      contiguous over (t, channel), so a term is one flat pass over L * channels element pairs: the difference is ONE
//                      fp32 subtraction, everything after it (|.|, square, the bce of the stop logits, every sum, the division by the
//                      channel count) is double.  Fixed order: a thread sums its stride, the wave a xor butterfly, thread f the 16 wave
//                      sums of field f in wave order -- no floating-point atomics, so a call is bitwise reproducible.
#include "kernels.h"
#include "device_utils.h"

#define GT_LOSS_THREADS 1024
#define GT_LOSS_WAVES (GT_LOSS_THREADS / GT_WAVE)
#define GT_LOSS_FIELDS 6

__device__ __forceinline__ double gt_wave_sum_d(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(GT_LOSS_THREADS) void gt_losses_kernel(LossArgs P) {
    __shared__ double wsum[GT_LOSS_WAVES][GT_LOSS_FIELDS];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = P.Tq - 1;
    const int64_t Tf = (int64_t)P.S * P.r;                  // prediction frames per utterance (>= T: frames t >= T are never read)
    const int L = P.mel_len ? min(max((int)P.mel_len[b], 0), T) : T;
    const int Ls = P.spec_len ? min(max((int)P.spec_len[b], 0), T) : T;
    double acc[GT_LOSS_FIELDS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};

    {   // fields 0-2: the pre-net and the post-net mel against teacher[b, 1:1+L]
        const float* tg = P.teacher + ((int64_t)b * P.Tq + 1) * P.mel_dim;
        const float* pre = P.pre_mel + (int64_t)b * Tf * P.mel_dim;
        const float* mel = P.mel + (int64_t)b * Tf * P.mel_dim;
        const int64_t n = (int64_t)L * P.mel_dim;
        for (int64_t i = tid; i < n; i += GT_LOSS_THREADS) {
            const float t = tg[i];
            const double d0 = (double)__fsub_rn(t, pre[i]), d1 = (double)__fsub_rn(t, mel[i]);
            acc[0] += fabs(d0);
            acc[1] += fabs(d1);
            acc[2] += d1 * d1;
        }
    }
    {   // field 3: sigmoid cross entropy of every step, label 1 while s < ceil(mel_length / r) (Model.py:227-234: not masked)
        const float* st = P.stop + (int64_t)b * P.S;
        int64_t going = P.S;
        if (P.mel_len) going = P.mel_len[b] > 0 ? ((int64_t)P.mel_len[b] + P.r - 1) / P.r : 0;
        for (int s = tid; s < P.S; s += GT_LOSS_THREADS) {
            const double x = (double)st[s], z = s < going ? 1.0 : 0.0;
            acc[3] += (x > 0.0 ? x : 0.0) - x * z + log1p(exp(-fabs(x)));
        }
    }
    if (P.spec && P.spec_target) {   // fields 4-5: the vocoder's spectrogram against spec_target[b, 1:1+Ls]
        const float* tg = P.spec_target + ((int64_t)b * P.Tq + 1) * P.spec_dim;
        const float* sp = P.spec + (int64_t)b * Tf * P.spec_dim;
        const int64_t n = (int64_t)Ls * P.spec_dim;
        for (int64_t i = tid; i < n; i += GT_LOSS_THREADS) {
            const double d = (double)__fsub_rn(tg[i], sp[i]);
            acc[4] += fabs(d);
            acc[5] += d * d;
        }
    }
#pragma unroll
    for (int f = 0; f < GT_LOSS_FIELDS; ++f) {
        const double w = gt_wave_sum_d(acc[f]);
        if (lane == 0) wsum[wave][f] = w;
    }
    __syncthreads();
    if (tid < GT_LOSS_FIELDS) {
        double t = wsum[0][tid];
        for (int w = 1; w < GT_LOSS_WAVES; ++w) t += wsum[w][tid];
        if (tid < 3) t /= (double)P.mel_dim;
        else if (tid > 3) t /= (double)P.spec_dim;
        P.losses[(int64_t)b * GT_LOSS_FIELDS + tid] = t;
    }
}

hipError_t gt_launch_losses(const LossArgs& a, hipStream_t stream) {
    if (!a.pre_mel || !a.mel || !a.stop || !a.teacher || !a.losses) return hipErrorInvalidValue;
    if (a.B < 1 || a.S < 1 || a.r < 1 || a.Tq < 2 || (int64_t)a.S * a.r < a.Tq - 1 || a.mel_dim < 1 || a.spec_dim < 1)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(gt_losses_kernel, dim3(a.B), dim3(GT_LOSS_THREADS), 0, stream, a);
    return hipGetLastError();
}
