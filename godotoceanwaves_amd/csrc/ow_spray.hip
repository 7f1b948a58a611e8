// ow_spray.hip -- the two kernels of a sea-spray step (ow_spray.h holds the arithmetic, which tests/spray/ also compiles as plain C++; the
// kernels are held to that build bit for bit).  Built with -ffp-contract=off, like ow_consumer.hip.
//
//   k_spray_step     one lane per particle, 256 lanes per block: restart, start(), process(); the 48-byte state and the 64-byte instance go
//                    out as 16-byte vector stores.  Only a lane that reaches :80 or :98 touches the maps, and a lane whose particle neither
//                    restarts nor is ACTIVE writes nothing.  Each wave ballots its live lanes; the block writes its live count, each wave's
//                    base inside the block and :89's two outcome counts to the per-block words.
//   k_spray_compact  each block sums the live counts of the blocks before it (a wave-strided load and a cross-lane reduction), ballots its
//                    own live lanes again from the flags and writes their indices at base + wave base + rank (the rank: the ballot's bits
//                    below the lane).  The last block writes live_count and adds the step's outcome counts to the emitter's totals.
//
// No block waits for another: the ascending order comes from the two launches, not from look-back, flags or atomics.
#include <hip/hip_runtime.h>

#include "ow_kernels.h"

namespace ow {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// bits of `mask` below this lane
__device__ __forceinline__ uint32_t rank_below(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__global__ void __launch_bounds__(kSprayBlock) k_spray_step(const u16x4 *disp, const u16x4 *norm, int n, int cascades, SurfaceScales scales,
                                                            SprayParams P, SprayClock K, SprayParticle *particles, SprayInstance *instances,
                                                            uint32_t *block_words) {
    __shared__ uint32_t wave_counts[3][kSprayBlock / 64];
    const uint32_t i = blockIdx.x * kSprayBlock + threadIdx.x;
    const int wave = (int)threadIdx.x >> 6;
    bool live = false;
    int spawn = 0;
    if (i < P.amount) {
        struct StateWords {
            u32x4 v[sizeof(SprayParticle) / 16];
        };
        struct InstanceWords {
            u32x4 v[sizeof(SprayInstance) / 16];
        };
        u32x4 *sp = (u32x4 *)(particles + i);
        StateWords sw;
        for (int k = 0; k < (int)(sizeof(SprayParticle) / 16); ++k) sw.v[k] = sp[k];
        SprayParticle s = __builtin_bit_cast(SprayParticle, sw);
        SprayInstance o;
        const SprayLane r = spray_lane(disp, norm, n, cascades, scales, P, K, i, s, o);
        live = r.live;
        spawn = r.spawn;
        if (r.wrote) {
            sw = __builtin_bit_cast(StateWords, s);
            for (int k = 0; k < (int)(sizeof(SprayParticle) / 16); ++k) sp[k] = sw.v[k];
            const InstanceWords iw = __builtin_bit_cast(InstanceWords, o);
            u32x4 *ip = (u32x4 *)(instances + i);
            for (int k = 0; k < (int)(sizeof(SprayInstance) / 16); ++k) ip[k] = iw.v[k];
        }
    }
    const uint64_t m_live = __ballot(live), m_spawned = __ballot(spawn == 1), m_rejected = __ballot(spawn == 2);
    if ((threadIdx.x & 63) == 0) {
        wave_counts[0][wave] = (uint32_t)__popcll(m_live);
        wave_counts[1][wave] = (uint32_t)__popcll(m_spawned);
        wave_counts[2][wave] = (uint32_t)__popcll(m_rejected);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t w[kSprayBlockWords];
        uint32_t base = 0, spawned = 0, rejected = 0;
        for (int k = 0; k < kSprayBlock / 64; ++k) {
            w[1 + k] = base;
            base += wave_counts[0][k];
            spawned += wave_counts[1][k];
            rejected += wave_counts[2][k];
        }
        w[0] = base;
        w[5] = spawned;
        w[6] = rejected;
        w[7] = 0u;
        u32x4 *dst = (u32x4 *)(block_words + (size_t)blockIdx.x * kSprayBlockWords);
        dst[0] = u32x4{w[0], w[1], w[2], w[3]};
        dst[1] = u32x4{w[4], w[5], w[6], w[7]};
    }
}

// the sum of v over the block's 256 lanes, in every lane (integers: the order does not matter)
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t *lds) {
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    __syncthreads();  // the previous use of lds is over
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return lds[0] + lds[1] + lds[2] + lds[3];
}

__global__ void __launch_bounds__(kSprayBlock) k_spray_compact(const SprayParticle *particles, uint32_t amount, const uint32_t *block_words,
                                                               uint32_t *draw_list, uint32_t *live_count, uint64_t *totals) {
    __shared__ uint32_t lds[kSprayBlock / 64];
    const uint32_t b = blockIdx.x, blocks = gridDim.x;
    const bool last = b + 1 == blocks;
    uint32_t before = 0;
    for (uint32_t k = threadIdx.x; k < b; k += kSprayBlock) before += block_words[(size_t)k * kSprayBlockWords];
    const uint32_t base = block_sum(before, lds);
    const uint32_t i = b * kSprayBlock + threadIdx.x;
    const uint32_t want = kSprayActive | kSprayHasStarted;
    const bool live = i < amount && (particles[i].flags & want) == want;
    const uint64_t mask = __ballot(live);
    if (live) {
        const uint32_t at = base + block_words[(size_t)b * kSprayBlockWords + 1 + (threadIdx.x >> 6)] + rank_below(mask);
        if (at < amount) draw_list[at] = i;  // always: the counts are those of these flags
    }
    if (last) {
        uint32_t spawned = 0, rejected = 0;
        for (uint32_t k = threadIdx.x; k < blocks; k += kSprayBlock) {
            spawned += block_words[(size_t)k * kSprayBlockWords + 5];
            rejected += block_words[(size_t)k * kSprayBlockWords + 6];
        }
        spawned = block_sum(spawned, lds);
        rejected = block_sum(rejected, lds);
        if (threadIdx.x == 0) {
            *live_count = base + block_words[(size_t)b * kSprayBlockWords];
            totals[0] += spawned;  // this launch is alone on these words: the steps of an emitter are ordered by its context's stream
            totals[1] += rejected;
        }
    }
}

}  // namespace

hipError_t launch_spray_step(int n, int cascades, const DeviceBuffers &buf, const SprayArrays &A, const SurfaceScales &scales, const SprayParams &P,
                             const SprayClock &K, hipStream_t s) {
    const unsigned blocks = (P.amount + kSprayBlock - 1) / kSprayBlock;
    hipLaunchKernelGGL(k_spray_step, dim3(blocks), dim3(kSprayBlock), 0, s, buf.disp, buf.norm, n, cascades, scales, P, K, A.particles, A.instances,
                       A.block_words);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_spray_compact, dim3(blocks), dim3(kSprayBlock), 0, s, A.particles, P.amount, A.block_words, A.draw_list, A.live_count, A.totals);
    return hipGetLastError();
}

}  // namespace ow
