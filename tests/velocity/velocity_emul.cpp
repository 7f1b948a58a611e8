// velocity_emul.cpp -- TEST INFRASTRUCTURE: steps the lanes of one block through the lane-level code of the velocity kernels
// (godotoceanwaves_amd/csrc/ow_velocity_kernels.h compiled as plain C++) on the CPU, phase by phase: every loop over the lanes below is
// what the lanes of k_velocity_pass1 / k_velocity_pass2 do between two __syncthreads().  The per-element load (vel_load), the stage
// functions in vel_row_fft's order, the S indexing and the per-texel epilogue (vel_texel) are the kernels' own; only the barriers and the
// global pointers are restated here.  Never shipped, never linked into libocean_waves.so.
#include <cmath>
#include <cstring>
#include <vector>

#include "ow_velocity_kernels.h"

using namespace ow;

namespace {

// tw[m] = exp(2 pi i m / n) as k_velocity_twiddles builds it: FP64 (sincospi: exact at the quarter turns), rounded once
void fill_twiddles(int n, std::vector<cplx> &tw) {
    tw.resize(n);
    const int q = n / 4;
    for (int m = 0; m < n; ++m) {
        const int r = m % q;
        double c = 1.0, s = 0.0;
        if (r != 0) {
            const double x = 2.0 * 3.14159265358979323846 * (double)r / (double)n;
            c = std::cos(x);
            s = std::sin(x);
        }
        switch (m / q) {
            case 0: tw[m] = cplx{(float)c, (float)s}; break;
            case 1: tw[m] = cplx{(float)-s, (float)c}; break;
            case 2: tw[m] = cplx{(float)-c, (float)-s}; break;
            default: tw[m] = cplx{(float)s, (float)-c}; break;
        }
    }
}

template <int N>
struct Block {
    using P = VelPlan<N>;
    static constexpr int T = P::T, W = P::W, NT = P::THREADS;
    std::vector<cplx> lds = std::vector<cplx>(W * P::STRIDE), tw;
    cplx va[NT][16], vb[NT][16];
    Block() { fill_twiddles(N, tw); }
    static int w_of(int l) { return l % W; }
    static int j_of(int l) { return l / W; }
    cplx *row(int l) { return lds.data() + w_of(l) * P::STRIDE; }

    // one exchange of vel_row_fft: the statements between two barriers are one loop over the lanes
    template <int R, int NS>
    void exchange() {
        for (int l = 0; l < NT; ++l) {
            vel_stage_butterflies<N, R, NS>(va[l], j_of(l), tw.data());
            vel_stage_butterflies<N, R, NS>(vb[l], j_of(l), tw.data());
            vel_stage_write<N, R, NS>(va[l], j_of(l), row(l));
        }
        for (int l = 0; l < NT; ++l) vel_stage_read<N>(va[l], j_of(l), row(l));
        for (int l = 0; l < NT; ++l) vel_stage_write<N, R, NS>(vb[l], j_of(l), row(l));
        for (int l = 0; l < NT; ++l) vel_stage_read<N>(vb[l], j_of(l), row(l));
    }
    void row_fft() {  // vel_row_fft<N>
        constexpr int R0 = P::R0;
        exchange<R0, 1>();
        if constexpr (R0 * 16 < N) exchange<16, R0>();
        constexpr int NSL = N / 16;
        for (int l = 0; l < NT; ++l) {
            vel_stage_butterflies<N, 16, NSL>(va[l], j_of(l), tw.data());
            vel_stage_butterflies<N, 16, NSL>(vb[l], j_of(l), tw.data());
        }
    }
};

// both passes of one layer.  inter (or null): the pass-1 intermediate un-tiled to [layer][ky][y] complex; layer: [y][x] RGBA16F
template <int N>
void layer(const cplx *h0, const float *omega, float tile_x, float tile_y, float time, cplx *inter, u16x4 *out) {
    using B = Block<N>;
    constexpr int T = B::T, W = B::W, NT = B::NT;
    const size_t plane = (size_t)N * N;
    std::vector<cplx> scratch(2 * plane);
    cplx *sa = scratch.data(), *sb = sa + plane;
    static B blk;
    for (int bx = 0; bx < N / W; ++bx) {  // k_velocity_pass1, block bx
        for (int l = 0; l < NT; ++l) {
            const int w = B::w_of(l), j = B::j_of(l), ky = bx * W + w;
            for (int m = 0; m < 16; ++m) {
                const VelPair v = vel_load<N>(ky, j + m * T, h0, omega, tile_x, tile_y, time);
                blk.va[l][m] = v.va;
                blk.vb[l][m] = v.vb;
            }
        }
        blk.row_fft();
        for (int l = 0; l < NT; ++l) {
            const int w = B::w_of(l), j = B::j_of(l);
            const size_t base = (size_t)bx * N * W + w;
            for (int k = 0; k < 16; ++k) {
                const size_t at = base + (size_t)(j + k * T) * W;
                sa[at] = blk.va[l][vel_slot<16>(k)];
                sb[at] = blk.vb[l][vel_slot<16>(k)];
            }
        }
    }
    if (inter)  // read as pass 2 reads S
        for (int ky = 0; ky < N; ++ky)
            for (int y = 0; y < N; ++y) {
                const size_t at = ((size_t)(ky / W) * N + y) * W + ky % W;
                inter[(size_t)ky * N + y] = sa[at];
                inter[plane + (size_t)ky * N + y] = sb[at];
            }
    for (int bx = 0; bx < N / W; ++bx) {  // k_velocity_pass2, block bx
        for (int l = 0; l < NT; ++l) {
            const int w = B::w_of(l), j = B::j_of(l), y = bx * W + w;
            for (int m = 0; m < 16; ++m) {
                const int ky = j + m * T;
                const size_t at = ((size_t)(ky / W) * N + y) * W + ky % W;
                blk.va[l][m] = sa[at];
                blk.vb[l][m] = sb[at];
            }
        }
        blk.row_fft();
        for (int l = 0; l < NT; ++l) {
            const int w = B::w_of(l), j = B::j_of(l), y = bx * W + w;
            u16x4 *row = out + (size_t)y * N;
            for (int k = 0; k < 16; ++k) {
                const int x = j + k * T;
                row[x] = vel_texel(blk.va[l][vel_slot<16>(k)], blk.vb[l][vel_slot<16>(k)], x, y);
            }
        }
    }
}

}  // namespace

extern "C" {
// h0: the layer's stored plane ([n][n] complex: h0(k)), omega [n][n]; inter: [2][n][n] complex or null; out: [n][n][4] halves
int velemul_layer(int n, const float *h0, const float *omega, float tile_x, float tile_y, float time, float *inter, uint16_t *out) {
    const cplx *h = (const cplx *)h0;
    cplx *it = (cplx *)inter;
    u16x4 *o = (u16x4 *)out;
    switch (n) {
        case 128: layer<128>(h, omega, tile_x, tile_y, time, it, o); return 0;
        case 256: layer<256>(h, omega, tile_x, tile_y, time, it, o); return 0;
        case 512: layer<512>(h, omega, tile_x, tile_y, time, it, o); return 0;
        case 1024: layer<1024>(h, omega, tile_x, tile_y, time, it, o); return 0;
        case 2048: layer<2048>(h, omega, tile_x, tile_y, time, it, o); return 0;
    }
    return 1;
}

// m = (cos, sin) of FP32 phases through expi_phase (on the CPU: sincos_phase)
void velemul_expi(int count, const float *ph, float *m) {
    for (int i = 0; i < count; ++i) {
        const cplx e = expi_phase(ph[i]);
        m[2 * i] = e.x;
        m[2 * i + 1] = e.y;
    }
}

void velemul_twiddles(int n, float *tw) {
    std::vector<cplx> t;
    fill_twiddles(n, t);
    std::memcpy(tw, t.data(), (size_t)n * sizeof(cplx));
}
}
