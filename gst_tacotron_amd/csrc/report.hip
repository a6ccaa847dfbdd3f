// Per-utterance seeds and the synthesis report: two kernels beside the decode step's own, both off the mel-frame hot path.
//
//   gt_fill_randomness_kernel   the keep masks and the SMA noise of a whole decode in the layouts injected randomness has, row b drawn
//                               from seeds[b] as a batch of ONE draws them at its row 0: an utterance's randomness then depends on
//                               its seed alone -- not on its row, the batch size or the padded width.  A sibling of gt_rng_fill_kernel
//                               (attention.hip), which draws a whole batch from one seed.
//   gt_utterance_report_kernel  what a decode's stop logits and alignments say about each utterance: where the stop token fired, whether
//                               the attention reached the last token, skipped, went back or stalled, and whether anything is not finite.
#include "kernels.h"
#include "device_utils.h"

__global__ __launch_bounds__(256) void gt_fill_randomness_kernel(const uint64_t* __restrict__ seeds, float* __restrict__ masks,
                                                                 float* __restrict__ noise, int steps, int B, int P0, int P1, int Tv,
                                                                 float drop_rate) {
    const int64_t per_step = (int64_t)B * (P0 + P1);
    const int64_t nmask = masks ? (int64_t)steps * per_step : 0;
    const int64_t nnoise = noise ? (int64_t)steps * B * Tv : 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nmask + nnoise; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < nmask) {
            const int t = (int)(i / per_step);
            const int64_t e = i - (int64_t)t * per_step;
            const bool second = e >= (int64_t)B * P0;
            const uint32_t idx = (uint32_t)(second ? e - (int64_t)B * P0 : e);         // b * P + column
            const uint32_t P = (uint32_t)(second ? P1 : P0);
            masks[i] = gt_drop_keep(seeds[idx / P], (uint32_t)t, second ? 1u : 0u, 0u, idx % P, P, drop_rate);
        } else {
            const int64_t j = i - nmask;
            const int t = (int)(j / ((int64_t)B * Tv));
            const uint32_t idx = (uint32_t)(j - (int64_t)t * B * Tv);                   // b * Tv + position
            const Philox4 r = gt_philox(seeds[idx / (uint32_t)Tv], idx % (uint32_t)Tv, (uint32_t)t, 0u, GT_RNG_NOISE);
            noise[j] = gt_normal(r.x, r.y);
        }
    }
}

hipError_t gt_launch_fill_randomness(const uint64_t* seeds, float* masks, float* noise, int steps, int B, int P0, int P1, int Tv,
                                     float drop_rate, hipStream_t stream) {
    if (!seeds || steps < 1 || B < 1 || Tv < 1 || P0 < 1 || P1 < 1) return hipErrorInvalidValue;
    const int64_t n = (masks ? (int64_t)steps * B * (P0 + P1) : 0) + (noise ? (int64_t)steps * B * Tv : 0);
    if (n == 0) return hipSuccess;
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(gt_fill_randomness_kernel, dim3(blocks), dim3(256), 0, stream, seeds, masks, noise, steps, B, P0, P1, Tv, drop_rate);
    return hipGetLastError();
}

// One workgroup of 16 waves per utterance.
//   1. s* = the first step with a negative stop logit: every thread keeps the first it meets on its stride, the workgroup the lowest.
//      From here on only the E = min(S, max(1, s*)) steps the utterance used are read.
//   2. In chunks of GT_REPORT_CHUNK steps (so that any S fits the LDS): a wave takes a step, its lanes stride the columns below n and keep
//      their first maximum, the wave keeps the larger value and between equal values the lower index -- gt_forced_durations_kernel's
//      rule -- and lane 0 writes a_s to the LDS and adds m_s to the wave's double.  Then a thread per step looks at its neighbour:
//      jump, back step, the bit of a_s in the visited bitmap, and -- at the first step of a run of equal values -- the run's length,
//      found by walking it.  The run that reaches the chunk's end is carried (carry_run, carry_prev) into the next chunk.
//   3. The four maxima / counts are combined with LDS atomics on integers (order-free), the 16 wave sums of m_s in wave order.
// Nothing is written to global memory but the utterance's own report row and focus.
#define GT_REPORT_THREADS 1024
#define GT_REPORT_WAVES (GT_REPORT_THREADS / GT_WAVE)
#define GT_REPORT_CHUNK 512

__device__ __forceinline__ int gt_nonfinite(float v) { return (__builtin_bit_cast(uint32_t, v) & 0x7F800000u) == 0x7F800000u ? 1 : 0; }

__global__ __launch_bounds__(GT_REPORT_THREADS) void gt_utterance_report_kernel(const float* __restrict__ stop, const float* __restrict__ align,
                                                                                const int32_t* __restrict__ tok_len,
                                                                                const float* __restrict__ mel, int32_t* __restrict__ report,
                                                                                float* __restrict__ focus, int S, int Tv, int r, int mel_dim) {
    extern __shared__ uint32_t seen[];          // (Tv + 31) / 32 words: bit j = some a_s is j
    __shared__ int32_t a_lds[GT_REPORT_CHUNK];
    __shared__ int32_t wfirst[GT_REPORT_WAVES];
    __shared__ double wsum[GT_REPORT_WAVES];
    __shared__ int32_t acc[6];                  // max a_s, max jump, back steps, max stall, visited, nonfinite
    __shared__ int32_t carry_prev, carry_run;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int words = (Tv + 31) >> 5;
    const float* stop_b = stop + (int64_t)b * S;

    for (int j = tid; j < words; j += GT_REPORT_THREADS) seen[j] = 0u;
    if (tid < 6) acc[tid] = 0;
    if (tid == 0) { carry_prev = 0; carry_run = 0; }
    int first = S;
    for (int s = tid; s < S; s += GT_REPORT_THREADS)
        if (stop_b[s] < 0.f) { first = s; break; }          // (a NaN is not below 0)
    for (int off = 32; off > 0; off >>= 1) first = min(first, __shfl_xor(first, off, 64));
    if (lane == 0) wfirst[wave] = first;
    __syncthreads();
    first = wfirst[0];
    for (int w = 1; w < GT_REPORT_WAVES; ++w) first = min(first, wfirst[w]);
    const int E = min(S, max(1, first));
    const int64_t frames = (int64_t)max(1, first) * r;
    int n = Tv;
    if (tok_len) n = max(1, min(Tv, (int)tok_len[b]));

    int nonfin = 0;
    for (int s = tid; s < E; s += GT_REPORT_THREADS) nonfin += gt_nonfinite(stop_b[s]);
    if (mel) {
        const float* mel_b = mel + (int64_t)b * S * r * mel_dim;
        for (int64_t i = tid; i < frames * mel_dim; i += GT_REPORT_THREADS) nonfin += gt_nonfinite(mel_b[i]);
    }

    double msum = 0.0;                          // (lane 0's copy is the wave's sum)
    int amax = 0, jump = 0, back = 0, stall = 0;
    for (int base = 0; base < E; base += GT_REPORT_CHUNK) {
        const int cnt = min(GT_REPORT_CHUNK, E - base);
        for (int i = wave; i < cnt; i += GT_REPORT_WAVES) {
            const float* a = align + ((int64_t)b * S + base + i) * Tv;
            float best = -INFINITY;
            int idx = n;                        // (n: nothing seen yet -- loses every tie)
            for (int j = lane; j < n; j += 64) {
                const float v = a[j];
                nonfin += gt_nonfinite(v);
                if (idx == n || v > best) { best = v; idx = j; }
            }
            for (int off = 32; off > 0; off >>= 1) {
                const float ov = __shfl_xor(best, off, 64);
                const int oi = __shfl_xor(idx, off, 64);
                if (oi < n && (idx >= n || ov > best || (ov == best && oi < idx))) { best = ov; idx = oi; }
            }
            // (n >= 1: lane 0 always holds column 0 at least, so idx < n in every lane after the butterfly)
            if (lane == 0) a_lds[i] = idx;
            msum += (double)best;
        }
        __syncthreads();
        int tail_run = 0;                       // > 0 in the one thread whose run reaches the chunk's end
        for (int i = tid; i < cnt; i += GT_REPORT_THREADS) {
            const int s = base + i, a = a_lds[i];
            const int prev = i > 0 ? a_lds[i - 1] : carry_prev;
            atomicOr(&seen[a >> 5], 1u << (a & 31));
            amax = max(amax, a);
            if (s > 0) {
                jump = max(jump, a - prev);
                back += a < prev ? 1 : 0;
            }
            const bool continues = s > 0 && a == prev;
            if (i == 0 && !continues) stall = max(stall, carry_run);           // (the run carried in ended with the chunk before)
            if (i == 0 || !continues) {
                int len = 1;
                while (i + len < cnt && a_lds[i + len] == a) ++len;
                const int total = len + (continues ? carry_run : 0);
                if (i + len == cnt) tail_run = total;
                else stall = max(stall, total);
            }
        }
        __syncthreads();                        // (carry_prev / carry_run have been read)
        if (tail_run > 0) { carry_run = tail_run; carry_prev = a_lds[cnt - 1]; }
        __syncthreads();
    }
    if (tid == 0) stall = max(stall, carry_run);
    for (int off = 32; off > 0; off >>= 1) nonfin += __shfl_xor(nonfin, off, 64);
    if (lane == 0) {
        atomicAdd(&acc[5], nonfin);
        wsum[wave] = msum;
    }
    atomicMax(&acc[0], amax);
    atomicMax(&acc[1], jump);
    if (back) atomicAdd(&acc[2], back);
    atomicMax(&acc[3], stall);
    __syncthreads();
    int vis = 0;
    for (int j = tid; j < words; j += GT_REPORT_THREADS) vis += __popc(seen[j]);
    if (vis) atomicAdd(&acc[4], vis);
    __syncthreads();
    if (tid == 0) {
        int32_t* out = report + (int64_t)b * 8;
        out[0] = first;
        out[1] = (int32_t)frames;
        out[2] = (n - 1) - acc[0];
        out[3] = acc[1];
        out[4] = acc[2];
        out[5] = acc[3];
        out[6] = acc[4];
        out[7] = acc[5];
        if (focus) {
            double t = wsum[0];
            for (int w = 1; w < GT_REPORT_WAVES; ++w) t += wsum[w];
            focus[b] = (float)(t / (double)E);
        }
    }
}

hipError_t gt_launch_utterance_report(const float* stop, const float* align, const int32_t* tok_len, const float* mel, int32_t* report,
                                      float* focus, int B, int S, int Tv, int r, int mel_dim, hipStream_t stream) {
    if (B < 1 || S < 1 || Tv < 1 || r < 1 || mel_dim < 1) return hipErrorInvalidValue;
    const size_t bitmap = (size_t)((Tv + 31) >> 5) * 4;
    if (bitmap > 32 * 1024) return hipErrorInvalidValue;    // (262144 tokens: far beyond what the attention kernels take)
    hipLaunchKernelGGL(gt_utterance_report_kernel, dim3(B), dim3(GT_REPORT_THREADS), bitmap, stream, stop, align, tok_len, mel, report, focus,
                       S, Tv, r, mel_dim);
    return hipGetLastError();
}
