// ow_velocity_kernels.h -- the water's velocity maps V = dD/dt on the device (include/ocean_waves.h ow_update_velocity).
//
// Layer c of V holds, at texel (x, y), the exact time derivatives of channels hx, hy, hz of layer c's displacement map (before
// displacement_scale), in m/s.  The maps are D = unpack(IFFT2(op(h))) with h = h0 m + conj(h0(-k)) conj(m), m = exp(i omega t)
// (spectrum_modulate.glsl:53-90); the transform and the operators are linear, so dD/dt = unpack(IFFT2(op(hdot))) with
//   hdot = i omega (h0 m - conj(h0(-k)) conj(m)).
// The operators are the maps' own: hx = i uy hdot, hy = hdot, hz = i ux hdot, packed two real fields per complex transform:
//   layer A = hx + i hy,  layer B = hz + i dhy_dx (dhy_dx = i ky hdot), the maps' own packed layers 0 and 1.  The spare half of B is not
//   left empty: on the Nyquist lines (kx or ky = -N/2, their own mirror) the operators are not Hermitian, so the two halves of a packed
//   transform leak into each other there, and the maps' hz carries that share of dhy_dx.  Packing B as the maps pack it makes V the
//   derivative of exactly what the maps hold (an empty half differs from it by up to 1 % of max|v_z|).
// The phase omega t and m are built with the FP32 operations of the maps' pass 1 (mul_rn, expi_phase), from the resident h0 / omega planes
// and the FP32 tile_length, depth and time words the layer's current maps were made with (ow_get_push_constants).  The transform is the
// maps' rows -> transpose -> rows (out = (N^2 ifft2(X))^T, no 1/N), the (-1)^(x+y) sign of fft_unpack.glsl:50 at the end.
//
// Two kernels per batch of up to kVelMaxBatch cascades, both with a row FFT of N/16 lanes x 16 points (Stockham, radix 16 with one radix
// 2 / 4 / 8 stage in front, exchanges through LDS, the twiddles from a table of exp(2 pi i m / N)):
//   k_velocity_pass1<N>: W spectrum rows ky per block: load + hdot + operators, the row transform along kx, stored in the tiled
//                        intermediate S[slot][layer][ky / W][y][ky % W] (a block writes one contiguous run per layer).
//   k_velocity_pass2<N>: W output rows y per block: reads S (W x W complex contiguous per ky / W), the transform along ky, the sign,
//                        RGBA16F out (one 8-byte vector store per texel).
// The intermediate is the pipeline's own: the frame scratch (T, pcol, rrow) may hold a speculated pass 1 and is never touched.
#pragma once

#include "ow_device.h"

namespace ow {

constexpr int kVelMaxBatch = 8;  // cascades per launch pair (the runtime bounds it further by the scratch it allocated, vel_batch)
// cascades per launch pair at map size n: 4 at 2048^2 keeps the intermediate at 256 MB, 8 below it (at most 128 MB)
constexpr int vel_batch(int n) { return n >= 2048 ? 4 : 8; }
// bytes of the intermediate of one cascade: two packed layers of N^2 complex FP32
constexpr size_t vel_scratch_bytes(int n) { return (size_t)n * (size_t)n * 2u * 8u; }

struct VelocityArgs {
    int count;                   // cascades of this launch (launch slots 0 .. count - 1)
    int cascade[kVelMaxBatch];   // which array layer each launch slot computes
    float tile_x[kVelMaxBatch];  // the FP32 words of the layer's modulate push constants (ow_get_push_constants: modulate[0], [1], [3])
    float tile_y[kVelMaxBatch];
    float time[kVelMaxBatch];
};

template <int N>
struct VelPlan {
    static constexpr int T = N / 16;                         // lanes per transform, 16 points each
    static constexpr int W = N >= 512 ? 4 : 2048 / N;        // rows per block (both passes): W x W complex runs in S >= 128 B
    static constexpr int THREADS = W * T;                    // 128 (N <= 512), 256 (1024), 512 (2048)
    static constexpr int R0 = N == 128 ? 8 : (N == 256 ? 16 : N / 256);  // first stage: 8 | 16 | 2 | 4 | 8, then radix 16
    static constexpr int STRIDE = N + 16;                    // LDS row stride (complex): the W rows of a wave's lanes land in different banks
};

// output k of Dft<R> (ow_device.h) sits in slot vel_slot<R>(k)
template <int R>
OW_HD constexpr int vel_slot(int k) {
    return R <= 4 ? k : (R == 8 ? 2 * (k % 4) + k / 4 : 4 * (k % 4) + k / 4);
}

// One Stockham stage of radix R over a length-N sequence with NS = product of the radices before it (inverse sign).  Lane j holds
// v[m] = in[j + m T], m = 0 .. 15 (the same elements before every stage); it runs the butterflies bf = j + q T, q < 16 / R, whose inputs
// are in[bf + r N / R] = v[q + r (16 / R)].  Outputs go to out[(bf / NS) NS R + bf % NS + k NS] through LDS (row `lds`, one layer), and
// the lane reads its next v[m] back.  The caller frames the exchange with barriers.
template <int N, int R, int NS>
OW_DEV void vel_stage_butterflies(cplx *v, int j, const cplx *__restrict__ tw) {
    constexpr int T = N / 16, Q = 16 / R;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        cplx u[R];
        const int bf = j + q * T;
#pragma unroll
        for (int r = 0; r < R; ++r) u[r] = v[q + r * Q];
        if constexpr (NS > 1) {
            const int e = (bf % NS) * (N / (NS * R));  // twiddle exp(2 pi i (bf % NS) r / (NS R)) = tw[e r]
#pragma unroll
            for (int r = 1; r < R; ++r) u[r] = cmul(u[r], tw[e * r]);
        }
        Dft<R>::run(u);
#pragma unroll
        for (int r = 0; r < R; ++r) v[q + r * Q] = u[r];
    }
}
template <int N, int R, int NS>
OW_DEV void vel_stage_write(const cplx *v, int j, cplx *lds) {
    constexpr int T = N / 16, Q = 16 / R;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int bf = j + q * T, base = (bf / NS) * NS * R + bf % NS;
#pragma unroll
        for (int k = 0; k < R; ++k) lds[base + k * NS] = v[q + vel_slot<R>(k) * Q];
    }
}
template <int N>
OW_DEV void vel_stage_read(cplx *v, int j, const cplx *lds) {
    constexpr int T = N / 16;
#pragma unroll
    for (int m = 0; m < 16; ++m) v[m] = lds[j + m * T];
}

template <int R_, int NS_>
struct VelStage {
    static constexpr int R = R_, NS = NS_;
};

// ---- pass 1, per element: spectrum texel (ky, kx) -> the two packed values -------------------------------------------------------------
struct VelPair {
    cplx va, vb;  // layer A = hx + i hy, layer B = hz + i dhy_dx
};
// The two packed values of spectrum texel (ky, kx) of one layer: h0c / omc are the layer's resident planes, tile_x / tile_y / time the FP32
// words of its modulate push constants.  (Plain C++ as well: tests/velocity/velocity_emul.cpp steps the lanes of a block through it.)
template <int N>
OW_DEV VelPair vel_load(int ky, int kx, const cplx *h0c, const float *omc, float tile_x, float tile_y, float time) {
    const cplx *a_row = h0c + (size_t)ky * N;
    const cplx *b_row = h0c + (size_t)((N - ky) % N) * N;  // the mirrored texel's row
    const float *o_row = omc + (size_t)ky * N;
    const float kyf = modulate_kcomp(ky, N, tile_y);
    const cplx a = a_row[kx], b = b_row[(N - kx) % N];
    const float om = o_row[kx];
    const cplx e = expi_phase(mul_rn(om, time));  // (cos, sin) of the maps' own FP32 phase (Pass1::modulate)
    // h0 m - conj(h0(-k)) conj(m) with the stored texel a = h0(k), b = h0(-k):
    //   g.re = (a.re - b.re) cos - (a.im - b.im) sin,  g.im = (a.re + b.re) sin + (a.im + b.im) cos;  hdot = i omega g
    const cplx pp = cadd(a, b), qq = csub(a, b);
    const float gre = qq.x * e.x - qq.y * e.y, gim = pp.x * e.y + pp.y * e.x;
    const cplx hd = cplx{-om * gim, om * gre};
    const float kxf = modulate_kcomp(kx, N, tile_x);
    const float k = sqrtf(kxf * kxf + kyf * kyf) + 1e-6f;  // spectrum_modulate.glsl:61-62
    const float ux = kxf / k, uy = kyf / k;
    const cplx ihd = cmuli(hd);
    const cplx hx = cscale(ihd, uy), hz = cscale(ihd, ux), gx = cscale(ihd, kyf);
    VelPair r;
    r.va = cplx{hx.x - hd.y, hx.y + hd.x};  // hx + i hy, hy = hdot
    r.vb = cplx{hz.x - gx.y, hz.y + gx.x};  // hz + i dhy_dx, dhy_dx = i ky hdot: the maps' layer 1, whose real part is hz
    return r;
}

// ---- pass 2, per texel -----------------------------------------------------------------------------------------------------------------
// texel (x, y) of the layer from the two transforms' values there: the sign, the three channels as halves, w = 0
OW_DEV u16x4 vel_texel(cplx A, cplx B, int x, int y) {
    const float s = ((x ^ y) & 1) ? -1.0f : 1.0f;  // fft_unpack.glsl:50
    const uint32_t w0 = f2h2(A.x * s, A.y * s), w1 = f2h2(B.x * s, 0.0f);
    u16x4 t;
    t.x = (uint16_t)(w0 & 0xffffu);
    t.y = (uint16_t)(w0 >> 16);
    t.z = (uint16_t)(w1 & 0xffffu);
    t.w = (uint16_t)(w1 >> 16);
    return t;
}

// ---- device only from here: the barriers of the row transform and the two kernels (the CPU emulation steps the stage functions itself) ----
#if OW_DEVICE_BUILD
// The row transform of both layers (a, b) of lane j: first stage R0 (NS = 1), then radix 16 until NS = N / 16.  After it, element
// j + k T of the result is in slot vel_slot<16>(k).  lds: this row's N (+ padding) complex, shared by the two layers in turn; every lane
// of the block runs this (barriers).
template <int N>
OW_DEV void vel_row_fft(cplx *a, cplx *b, int j, cplx *lds, const cplx *__restrict__ tw) {
    constexpr int R0 = VelPlan<N>::R0;
    auto exchange = [&](auto stage) {
        constexpr int R = decltype(stage)::R, NS = decltype(stage)::NS;
        vel_stage_butterflies<N, R, NS>(a, j, tw);
        vel_stage_butterflies<N, R, NS>(b, j, tw);
        vel_stage_write<N, R, NS>(a, j, lds);
        __syncthreads();
        vel_stage_read<N>(a, j, lds);
        __syncthreads();
        vel_stage_write<N, R, NS>(b, j, lds);
        __syncthreads();
        vel_stage_read<N>(b, j, lds);
        __syncthreads();
    };
    exchange(VelStage<R0, 1>{});
    if constexpr (R0 * 16 < N) exchange(VelStage<16, R0>{});  // N >= 512: a middle radix-16 stage
    // the last stage: its outputs stay in the lanes (element j + k T in slot vel_slot<16>(k), since bf = j < NS there)
    constexpr int NSL = N / 16;
    vel_stage_butterflies<N, 16, NSL>(a, j, tw);
    vel_stage_butterflies<N, 16, NSL>(b, j, tw);
}

// ---- pass 1: spectrum rows ky -> the row transform along kx -> S ------------------------------------------------------------------
// S of launch slot s, layer l: scratch + (2 s + l) N^2, entry ((ky / W) N + y) W + ky % W.
template <int N>
__global__ __launch_bounds__(VelPlan<N>::THREADS) void k_velocity_pass1(VelocityArgs args, const cplx *__restrict__ h0, const float *__restrict__ omega,
                                                                       const cplx *__restrict__ tw, cplx *__restrict__ scratch) {
    using P = VelPlan<N>;
    constexpr int T = P::T, W = P::W;
    __shared__ __attribute__((aligned(16))) cplx lds[W * P::STRIDE];
    const int w = (int)threadIdx.x % W, j = (int)threadIdx.x / W;
    const int slot = blockIdx.y;
    const int ky = (int)blockIdx.x * W + w;
    const int c = args.cascade[slot];
    const float time = args.time[slot];
    const size_t plane = (size_t)N * N;
    cplx va[16], vb[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) {
        const int kx = j + m * T;
        const VelPair v = vel_load<N>(ky, kx, h0 + c * plane, omega + c * plane, args.tile_x[slot], args.tile_y[slot], time);
        va[m] = v.va;
        vb[m] = v.vb;
    }
    vel_row_fft<N>(va, vb, j, lds + w * P::STRIDE, tw);
    cplx *sa = scratch + (size_t)(2 * slot) * plane, *sb = sa + plane;
    const size_t base = (size_t)blockIdx.x * N * W + w;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const size_t at = base + (size_t)(j + k * T) * W;  // y = j + k T
        sa[at] = va[vel_slot<16>(k)];
        sb[at] = vb[vel_slot<16>(k)];
    }
}

// ---- pass 2: S rows y -> the transform along ky -> sign -> RGBA16F ------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(VelPlan<N>::THREADS) void k_velocity_pass2(VelocityArgs args, const cplx *__restrict__ scratch, const cplx *__restrict__ tw,
                                                                       u16x4 *__restrict__ vel) {
    using P = VelPlan<N>;
    constexpr int T = P::T, W = P::W;
    __shared__ __attribute__((aligned(16))) cplx lds[W * P::STRIDE];
    const int w = (int)threadIdx.x % W, j = (int)threadIdx.x / W;
    const int slot = blockIdx.y;
    const int y = (int)blockIdx.x * W + w;
    const size_t plane = (size_t)N * N;
    const cplx *sa = scratch + (size_t)(2 * slot) * plane, *sb = sa + plane;
    cplx va[16], vb[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) {
        const int ky = j + m * T;
        const size_t at = ((size_t)(ky / W) * N + y) * W + ky % W;
        va[m] = sa[at];
        vb[m] = sb[at];
    }
    vel_row_fft<N>(va, vb, j, lds + w * P::STRIDE, tw);
    u16x4 *row = vel + (size_t)args.cascade[slot] * plane + (size_t)y * N;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int x = j + k * T;
        row[x] = vel_texel(va[vel_slot<16>(k)], vb[vel_slot<16>(k)], x, y);
    }
}
#endif

}  // namespace ow
