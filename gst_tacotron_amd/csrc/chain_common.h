// The per-utterance attention chain of the decode step, once: the small reductions, the additive score of a memory row, the alignment
// functions (SMA update, BMA safe-cumprod chain, LSA softmax) and the context row loop.  Callers: the four-kernel path (attention.hip: the
// alignment functions only -- its score and context passes sum in another order and serve as the independent reference), the fused front
// kernel's two utterance paths (front_body.h, front_lean.h) and the persistent decode kernel (persist_decode.hip: everything but the
// score row, which it keeps in registers).  Their results are compared bitwise, so nothing in here may depend on which caller it serves:
// what one caller needs and the others do not goes through `emit` or stays at the call site.
#pragma once
#include <hip/hip_runtime.h>
#include "device_utils.h"

// acc += x * r, one fused multiply-add per component.  EXPLICIT: `a += b * c` leaves the fusion to the optimiser, call site by call
// site; the chain is called from three fused kernels (general, lean, persistent) whose outputs are compared bitwise.
__device__ __forceinline__ void gt_fma4(float4& acc, const float x, const float4& r) {
    acc.x = __builtin_fmaf(x, r.x, acc.x); acc.y = __builtin_fmaf(x, r.y, acc.y);
    acc.z = __builtin_fmaf(x, r.z, acc.z); acc.w = __builtin_fmaf(x, r.w, acc.w);
}

// sum of the k-part partials of one column; 8 independent LDS reads in flight per round (a plain
// `z += partial[...]` loop serialises ~100-cycle LDS round trips: 32 of them cost >1 us per phase)
__device__ __forceinline__ float reduce_partial(const float* partial, int kparts, int N, int col) {
    float z = 0.f;
    int p = 0;
    for (; p + 8 <= kparts; p += 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = partial[(size_t)(p + j) * N + col];
        z += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
    for (; p < kparts; ++p) z += partial[(size_t)p * N + col];
    return z;
}

// Additive score of one memory row (Steps.py:126-152), the fused front kernel's form: L lanes per row of the LDS tile (row stride LD),
// each reading its NP 16-byte pieces of the row, of the query and of v; returns sum_a v[a] * tanh(q[a] + row[a]) in every lane of the
// row's group.
template <int L, int NP, int LD>
__device__ __forceinline__ float gt_score_row(const float* tile, const int row, const float* qs, const float* vs, const int li) {
    f32x2 s2 = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int a0 = 4 * (li + L * j);
        const float4 m4 = *reinterpret_cast<const float4*>(tile + row * LD + a0);
        const float4 q4 = *reinterpret_cast<const float4*>(qs + a0);
        const float4 w4 = *reinterpret_cast<const float4*>(vs + a0);
        s2 = __builtin_elementwise_fma(f32x2{w4.x, w4.y}, gt_tanh2(f32x2{q4.x, q4.y} + f32x2{m4.x, m4.y}), s2);
        s2 = __builtin_elementwise_fma(f32x2{w4.z, w4.w}, gt_tanh2(f32x2{q4.z, q4.w} + f32x2{m4.z, m4.w}), s2);
    }
    return gt_row_sum<L>(s2.x + s2.y);
}

// The two clips of the reference's safe_cumprod (Steps.py:183-199): clip(1 - p, tiny, 1) in front of the log, with tiny the smallest
// normal float32, and clip(cumprod, 1e-10, 1) in front of the division.
constexpr float GT_BMA_TINY = 1.17549435e-38f;
constexpr float GT_BMA_CP_MIN = 1e-10f;

// SMA update (Steps.py:215-229) of a position t > 0: own = pv[t] * p[t], the position's own term (all there is at position 0, which
// has no left neighbour).  The fma is EXPLICIT: `a*b + c*d` may contract around either product, call site by call site, and the
// callers must round alike.
__device__ __forceinline__ float gt_sma(const float own, const float pv_prev, const float p_prev) {
    return __builtin_fmaf(pv_prev, 1.f - p_prev, own);
}

// BMA (Steps.py:168-199) on ONE FULLY ACTIVE wave: sc holds p = sigmoid(score + noise), pv the previous alignment;
// cp = exp(exclusive_cumsum(log(clip(1 - p, tiny, 1)))), al = p * cp * cumsum(pv / clip(cp, 1e-10, 1)).  A serial run of ceil(Tv/64)
// positions per lane and a wave scan, twice.  `emit(t, al[t])`: the caller's side store per position.
template <class Emit>
__device__ __forceinline__ void gt_bma_align_wave(const float* sc, const float* pv, float* al, const int Tv, const int lane, Emit emit) {
    const int per = (Tv + 63) / 64;
    const int t0 = lane * per, t1 = min(Tv, t0 + per);
    float run = 0.f;
    for (int t = t0; t < t1; ++t) run += logf(fminf(fmaxf(1.f - sc[t], GT_BMA_TINY), 1.f));
    float base = gt_wave_incl_scan(run, lane) - run;
    for (int t = t0; t < t1; ++t) {
        const float lg = logf(fminf(fmaxf(1.f - sc[t], GT_BMA_TINY), 1.f));
        al[t] = expf(base);            // exclusive cumprod
        base += lg;
    }
    run = 0.f;
    for (int t = t0; t < t1; ++t) run += pv[t] / fminf(fmaxf(al[t], GT_BMA_CP_MIN), 1.f);
    base = gt_wave_incl_scan(run, lane) - run;
    for (int t = t0; t < t1; ++t) {
        base += pv[t] / fminf(fmaxf(al[t], GT_BMA_CP_MIN), 1.f);
        al[t] = sc[t] * al[t] * base;
        emit(t, al[t]);
    }
}

// LSA: softmax (or the smoothing normalisation, Layers.py:426-444) of the scores sc over the Tv positions on one fully active wave,
// a serial run per lane.  `emit(t, al[t])`: the caller's side store per position (the location state, the context pass's copy).
template <class Emit>
__device__ __forceinline__ void gt_softmax_align_wave(const float* sc, float* al, const int Tv, const int lane, const bool smoothing, Emit emit) {
    const int per = (Tv + 63) / 64;
    const int t0 = lane * per, t1 = min(Tv, t0 + per);
    float mx = -INFINITY;
    for (int t = t0; t < t1; ++t) mx = fmaxf(mx, sc[t]);
    mx = gt_wave_max(mx);
    float sum = 0.f;
    for (int t = t0; t < t1; ++t) {
        const float e = smoothing ? 1.f / (1.f + expf(-sc[t])) : expf(sc[t] - mx);
        al[t] = e;
        sum += e;
    }
    sum = gt_wave_sum(sum);
    const float inv = 1.f / sum;
    for (int t = t0; t < t1; ++t) {
        al[t] *= inv;
        emit(t, al[t]);
    }
}

// Context pass, channel ca over the rows cp, cp + G, .. < nr of a memory tile (row stride LD): two partial sums over alternating rows,
// an odd last row into the first.
template <int G, int LD>
__device__ __forceinline__ float gt_ctx_rows(const float* alc, const float* tile, const int ca, const int cp, const int nr) {
    float p0 = 0.f, p1 = 0.f;
    int t = cp;
    for (; t + G < nr; t += 2 * G) {
        p0 = __builtin_fmaf(alc[t], tile[t * LD + ca], p0);
        p1 = __builtin_fmaf(alc[t + G], tile[(t + G) * LD + ca], p1);
    }
    if (t < nr) p0 = __builtin_fmaf(alc[t], tile[t * LD + ca], p0);
    return p0 + p1;
}
