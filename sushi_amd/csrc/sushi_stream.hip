// sushi_amd/csrc/sushi_stream.hip -- gfx950 (MI355X, CDNA4): stream preparation and the C ABI of a prepared stream.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <memory>

#include "../../include/sushi_hip.h"
#include "sushi_common.hpp"
#include "sushi_internal.hpp"

namespace {

using namespace sushi;

// ------------------------------------------------------------------------------------------
// Stream preparation: centred float32 copy + float64 exclusive prefix sums of xc and xc^2.
// Three passes over blocks of PB samples (block totals -> scan of totals -> in-block scan).
// ------------------------------------------------------------------------------------------
constexpr int PB_THREADS = 256;
constexpr int PB_PER_THREAD = 16;
static_assert(PB == PB_THREADS * PB_PER_THREAD, "a block of the passes (stream_core.hpp: 4096 samples) is a workgroup's");

template <typename T> __device__ __forceinline__ float centred(T x);
template <> __device__ __forceinline__ float centred<float>(float x) { return x - 0.5f; }
template <> __device__ __forceinline__ float centred<uint8_t>(uint8_t x) { return (float)((int)x - 128); }

template <typename T>
__global__ __launch_bounds__(PB_THREADS)
void centre_blocksum_kernel(const T* __restrict__ raw, int64_t n, float* __restrict__ xc,
                            double* __restrict__ bs1, double* __restrict__ bs2) {
    __shared__ double r1[PB_THREADS / 64], r2[PB_THREADS / 64];
    const int64_t base = (int64_t)blockIdx.x * PB;
    double s1 = 0.0, s2 = 0.0;
#pragma unroll 4
    for (int k = 0; k < PB_PER_THREAD; ++k) {
        const int64_t e = base + (int64_t)k * PB_THREADS + threadIdx.x;   // coalesced
        if (e < n) {
            const T x = raw[e];
            const double u = (double)x;                                   // the sample as it is
            xc[e] = centred<T>(x);                                        // what the direct kernel multiplies
            s1 += u;
            s2 += u * u;
        }
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if ((threadIdx.x & 63) == 0) { r1[threadIdx.x >> 6] = s1; r2[threadIdx.x >> 6] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t1 = 0.0, t2 = 0.0;
        for (int w = 0; w < PB_THREADS / 64; ++w) { t1 += r1[w]; t2 += r2[w]; }
        bs1[blockIdx.x] = t1;
        bs2[blockIdx.x] = t2;
    }
}

// single workgroup: in-place exclusive scan of the per-block totals of NA arrays; entry [nb] of each
// receives the grand total, so that bs[b] = prefix sum at sample min(b * PB, n) for b = 0 .. nb
template <int NA>
__global__ __launch_bounds__(1024)
void scan_blocksums_kernel(double* __restrict__ bs, int stride, int nb) {
    __shared__ double wt[NA][16];
    __shared__ double carry[NA];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid < NA) carry[tid] = 0.0;
    __syncthreads();
    for (int base = 0; base < nb; base += 1024) {
        const int k = base + tid;
        double v[NA], e[NA], o[NA];
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            v[a] = k < nb ? bs[a * stride + k] : 0.0;
            double t;
            e[a] = wave_excl_scan(v[a], &t);
            if (lane == 0) wt[a][wv] = t;
        }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            o[a] = carry[a];
            for (int w = 0; w < wv; ++w) o[a] += wt[a][w];
            if (k < nb) bs[a * stride + k] = o[a] + e[a];
        }
        __syncthreads();
        if (tid == 1023) {
#pragma unroll
            for (int a = 0; a < NA; ++a) carry[a] = o[a] + e[a] + v[a];
        }
        __syncthreads();
    }
    if (tid < NA) bs[tid * stride + nb] = carry[tid];
}

// prefix sums s1 = sum x, s2 = sum x^2 of the samples as they are (float64, absolute: exact for uint8) and,
// for the FFT path's scoring, s2 again as float32 relative to the base of the sample's PB-block:
//     s2[e] = base2[e / PB] + urel[e]          (e = 0 .. n)
template <typename T>
__global__ __launch_bounds__(PB_THREADS)
void final_scan_kernel(const T* __restrict__ raw, int64_t n, const double* __restrict__ bs1,
                       const double* __restrict__ bs2, double* __restrict__ s1, double* __restrict__ s2,
                       float* __restrict__ urel, float* __restrict__ usrel) {
    // A thread scans PB_PER_THREAD consecutive samples, but global memory is touched a workgroup-wide row at a
    // time: samples come in and prefix values go out through a padded LDS tile (index + index / 16: the
    // 16-element runs of neighbouring threads start in different banks).
    __shared__ double tile[PB + PB / PB_PER_THREAD];
    __shared__ double w1[PB_THREADS / 64], w2[PB_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t blk = (int64_t)blockIdx.x * PB;
    auto pad = [](const int i) { return i + i / PB_PER_THREAD; };
#pragma unroll
    for (int k = 0; k < PB_PER_THREAD; ++k) {
        const int i = k * PB_THREADS + tid;                              // coalesced
        const int64_t e = blk + i;
        tile[pad(i)] = e < n ? (double)raw[e] : 0.0;
    }
    __syncthreads();
    double v[PB_PER_THREAD];
    double l1 = 0.0, l2 = 0.0;
#pragma unroll
    for (int k = 0; k < PB_PER_THREAD; ++k) {
        v[k] = tile[pad(tid * PB_PER_THREAD + k)];
        l1 += v[k];
        l2 += v[k] * v[k];
    }
    double t1, t2;
    double e1 = wave_excl_scan(l1, &t1);
    double e2 = wave_excl_scan(l2, &t2);
    if (lane == 0) { w1[wv] = t1; w2[wv] = t2; }
    __syncthreads();                                                     // also: everyone has read its samples
    for (int w = 0; w < wv; ++w) { e1 += w1[w]; e2 += w2[w]; }           // prefix inside the block, before the thread's run
    const double o1 = bs1[blockIdx.x], o2 = bs2[blockIdx.x];             // block bases
    if (blockIdx.x == 0 && tid == 0) {
        s1[0] = 0.0; s2[0] = 0.0;
        if (n % PB == 0) { urel[n] = 0.f; usrel[2 * n] = 0.f; usrel[2 * n + 1] = 0.f; }   // sample n opens a block of its own: base[n / PB] = total
    }
    // s1[e + 1], s2[e + 1] (inclusive sums) and urel[e] (exclusive, relative to the block), one array at a time
    {
        double r = e1;
#pragma unroll
        for (int k = 0; k < PB_PER_THREAD; ++k) { r += v[k]; tile[pad(tid * PB_PER_THREAD + k)] = o1 + r; }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PB_PER_THREAD; ++k) {
        const int i = k * PB_THREADS + tid;
        if (blk + i < n) s1[blk + i + 1] = tile[pad(i)];
    }
    __syncthreads();
    {
        double r = e2;
#pragma unroll
        for (int k = 0; k < PB_PER_THREAD; ++k) { r += v[k] * v[k]; tile[pad(tid * PB_PER_THREAD + k)] = o2 + r; }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PB_PER_THREAD; ++k) {
        const int i = k * PB_THREADS + tid;
        if (blk + i < n) s2[blk + i + 1] = tile[pad(i)];
    }
    __syncthreads();
    // urel[e] (exclusive, relative to the block) and the same for the sum of the samples (TM_CCOEFF_NORMED's window means:
    // s1[e] = base1[e / PB] + srel[e]); the pair goes out twice: urel alone (TM_SQDIFF_NORMED reads nothing else) and
    // interleaved as usrel[e] = (urel[e], srel[e]), so that TM_CCOEFF_NORMED's scoring takes both with ONE 8-byte load per
    // window end instead of two 4-byte ones
    struct f2 { float u, s; };
    f2* __restrict__ ftile = reinterpret_cast<f2*>(tile);
    {
        double r2 = e2, r1 = e1;
#pragma unroll
        for (int k = 0; k < PB_PER_THREAD; ++k) {
            ftile[pad(tid * PB_PER_THREAD + k)] = f2{(float)r2, (float)r1};
            r2 += v[k] * v[k];
            r1 += v[k];
        }
    }
    __syncthreads();
    f2* __restrict__ us = reinterpret_cast<f2*>(usrel);
#pragma unroll
    for (int k = 0; k < PB_PER_THREAD; ++k) {
        const int i = k * PB_THREADS + tid;
        // e == n inside this block (n % PB != 0): samples past the end are zeros, so the running sum there is the total
        if (blk + i <= n) {
            const f2 x = ftile[pad(i)];
            urel[blk + i] = x.u;
            us[blk + i] = x;
        }
    }
}

// s2 and s1 at every COARSE_G-th sample (entries past the end: the totals) -- a table small enough to live in the L2s, from which
// bound_kernel takes a lower bound of the window energies of a whole block pair
__global__ void coarse_prefix_kernel(const double* __restrict__ s1, const double* __restrict__ s2, int64_t n, int64_t nc,
                                     double* __restrict__ coarse) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < nc) {
        const int64_t e = j * COARSE_G < n ? j * COARSE_G : n;
        coarse[j] = s2[e];
        coarse[nc + j] = s1[e];
    }
}

// What the FFT path needs to know about a stream as a whole (sushi_fft.hip, "packed halves"): the constant its block
// spectra are centred by -- the stream's own mean, as a float: any constant is exact (sum T I = sum T (I - c) + c sum T),
// the mean keeps DC out of the products whatever level the data sits at -- and the largest centred energy of FFT_STEP + 1
// consecutive blocks (what one block pair's transform can hold at most: the scale of the packed products is derived
// from it).  One workgroup; bs2 / bs1 are the scanned block bases of sum x^2 / sum x.
__global__ __launch_bounds__(1024)
void fft_stats_kernel(const double* __restrict__ bs2, const double* __restrict__ bs1, int nb, int64_t n, double* __restrict__ stats) {
    __shared__ double red[16];
    const int tid = threadIdx.x;
    const double c = (double)(float)(bs1[nb] / (double)n);
    double emax = 0.0;
    for (int j = tid; j < nb; j += 1024) {
        const int je = min(j + FFT_STEP + 1, nb);
        const int64_t lo = (int64_t)j * PB, hi = min((int64_t)je * PB, n);
        const double e = (bs2[je] - bs2[j]) - 2.0 * c * (bs1[je] - bs1[j]) + c * c * (double)(hi - lo);
        emax = e > emax ? e : emax;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const double o = __shfl_down(emax, d, 64); emax = o > emax ? o : emax; }
    if ((tid & 63) == 0) red[tid >> 6] = emax;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w) emax = red[w] > emax ? red[w] : emax;
        stats[0] = emax;
        stats[1] = c;
    }
}

}  // namespace

using namespace sushi;

extern "C" {

int sushi_hip_abi_version(void) { return SUSHI_HIP_ABI_VERSION; }

const char* sushi_hip_strerror(int code) {
    switch (code) {
        case SUSHI_HIP_OK: return "ok";
        case SUSHI_HIP_EINVAL: return "invalid argument";
        case SUSHI_HIP_EALIGN: return "device pointer not aligned";
        case SUSHI_HIP_ELAUNCH: return "HIP launch failed";
        case SUSHI_HIP_ENOSPACE: return "buffer or workspace too small";
        case SUSHI_HIP_ENODEV: return "no gfx950 device";
        case SUSHI_HIP_ENOMEM: return "out of host memory";
        case SUSHI_HIP_EINTERNAL: return "internal error (a C++ exception was caught at the boundary)";
        default: return "unknown sushi_hip error";
    }
}

int sushi_hip_device_ok(void) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return SUSHI_HIP_ENODEV;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return SUSHI_HIP_ENODEV;
    const char* arch = prop.gcnArchName;
    // "gfx950:sramecc+:xnack-"
    if (arch[0] == 'g' && arch[1] == 'f' && arch[2] == 'x' && arch[3] == '9' && arch[4] == '5' && arch[5] == '0')
        return SUSHI_HIP_OK;
    return SUSHI_HIP_ENODEV;
}

double sushi_hip_centre(int dtype) { return dtype == SUSHI_HIP_U8 ? 128.0 : 0.5; }

size_t sushi_hip_stream_bytes(int64_t n, int dtype, int searchable) { return stream_bytes(n, dtype, searchable); }

int sushi_hip_stream_create(const void* raw_dev, int dtype, int64_t n, int searchable, void* mem_dev, size_t mem_bytes,
                            void* hip_stream, SushiHipStream** out) { return c_boundary([&]() -> int {
    if (!raw_dev || !mem_dev || !out || n <= 0) return SUSHI_HIP_EINVAL;
    if (!stream_dtype_ok(dtype)) return SUSHI_HIP_EINVAL;
    if (((uintptr_t)mem_dev & 255) || (dtype == SUSHI_HIP_F32 && ((uintptr_t)raw_dev & 3))) return SUSHI_HIP_EALIGN;
    const StreamLayout l = stream_layout(n, searchable);
    if (mem_bytes < l.total) return SUSHI_HIP_ENOSPACE;
    if (l.nb > 0x7ffffffe) return SUSHI_HIP_EINVAL;
    const int nb = (int)l.nb;
    std::unique_ptr<SushiHipStream> s(new SushiHipStream());
    fill_stream(*s, raw_dev, dtype, n, mem_dev, l);
    hipStream_t st = (hipStream_t)hip_stream;
    double* bs2 = s->base;                       // block bases of sum x^2 (what the FFT path's scoring reads)
    double* bs1 = s->base1;                      // block bases of sum x
    if (dtype == SUSHI_HIP_F32)
        hipLaunchKernelGGL(centre_blocksum_kernel<float>, dim3(nb), dim3(PB_THREADS), 0, st,
                           (const float*)raw_dev, n, s->xc, bs1, bs2);
    else
        hipLaunchKernelGGL(centre_blocksum_kernel<uint8_t>, dim3(nb), dim3(PB_THREADS), 0, st,
                           (const uint8_t*)raw_dev, n, s->xc, bs1, bs2);
    int rc = launch_ok();
    if (rc == SUSHI_HIP_OK) {
        hipLaunchKernelGGL(scan_blocksums_kernel<2>, dim3(1), dim3(1024), 0, st, s->base, nb + 1, nb);
        rc = launch_ok();
    }
    if (rc == SUSHI_HIP_OK) {
        if (dtype == SUSHI_HIP_F32)
            hipLaunchKernelGGL(final_scan_kernel<float>, dim3(nb), dim3(PB_THREADS), 0, st, (const float*)raw_dev, n,
                               (const double*)bs1, (const double*)bs2, s->s1, s->s2, s->urel, s->usrel);
        else
            hipLaunchKernelGGL(final_scan_kernel<uint8_t>, dim3(nb), dim3(PB_THREADS), 0, st, (const uint8_t*)raw_dev, n,
                               (const double*)bs1, (const double*)bs2, s->s1, s->s2, s->urel, s->usrel);
        rc = launch_ok();
    }
    if (rc == SUSHI_HIP_OK) {
        hipLaunchKernelGGL(fft_stats_kernel, dim3(1), dim3(1024), 0, st, (const double*)bs2, (const double*)bs1, nb, n, s->stats);
        rc = launch_ok();
    }
    if (rc == SUSHI_HIP_OK) {
        hipLaunchKernelGGL(coarse_prefix_kernel, dim3((unsigned)((s->nc + 255) / 256)), dim3(256), 0, st, (const double*)s->s1,
                           (const double*)s->s2, n, s->nc, s->coarse);
        rc = launch_ok();
    }
    if (rc == SUSHI_HIP_OK && searchable)
        rc = sushi_hip_stream_add_spectra(s.get(), s->mem + l.spec, mem_bytes - l.spec, hip_stream);
    if (rc != SUSHI_HIP_OK) return rc;
    *out = s.release();
    return SUSHI_HIP_OK;
}); }

int sushi_hip_stream_view(const SushiHipStream* s, int which, const void** ptr_dev, size_t* bytes) {
    if (!s || !ptr_dev || !bytes) return SUSHI_HIP_EINVAL;
    return stream_view(*s, which, ptr_dev, bytes);
}

void sushi_hip_stream_destroy(SushiHipStream* s) { delete s; }

}  // extern "C"
