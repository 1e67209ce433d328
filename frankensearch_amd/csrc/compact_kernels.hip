// compact_kernels.hip — the vector pass of rewrite_index (crates/frankensearch-index/src/lib.rs:3003-3045) on the device-resident slab.
//
// compact() and vacuum() write the surviving rows of the old slab, byte for byte, into a new one (WAL rows, already encoded into the
// slab's format, come from a block of their own).  Which rows survive is the host's plan; the device gets it as RUNS (kernels.hpp):
// at most tombstones + WAL entries + 1 of them, not one word per row.  The kernel is a segmented copy:
//
//   * a wave owns kCompactWaveBytes contiguous destination bytes; one binary search over the runs' destination offsets finds the
//     run its first byte lies in, then it walks the runs until its range ends;
//   * inside a run source and destination differ by a constant shift — (rows dropped so far) x row bytes.  When that shift and both
//     ends are multiples of 16 the wave moves 16 bytes per lane, 1 KB contiguous per instruction, four instructions in flight; else
//     the widest unit the shift allows (8, 4 or 2 bytes: rows of 8, 86, 172 or 200 bytes are in the contract), with the few bytes
//     before the first and after the last aligned unit moved as 2-byte elements (every offset is a multiple of the element size);
//   * every offset is 64-bit: slabs beyond 4 GiB are the normal case.
//
// One pass, no reuse: no LDS, nothing to keep in a cache.  NT = the stores carry the non-temporal hint (measured, not assumed:
// DESIGN 3.12).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"

namespace fsgpu {

namespace {

typedef uint32_t cu32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t cu32x2 __attribute__((ext_vector_type(2)));

template <typename V, bool NT>
__device__ __forceinline__ void put(V* p, V v) {
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// n units of V from s to d (both aligned to V), the wave's 64 lanes side by side, four units per lane in flight
template <typename V, bool NT>
__device__ __forceinline__ void copy_units(const unsigned char* __restrict__ s, unsigned char* __restrict__ d, uint64_t n, uint32_t lane) {
    const V* sp = reinterpret_cast<const V*>(s);
    V* dp = reinterpret_cast<V*>(d);
    uint64_t i = lane;
    for (; i + 192 < n; i += 256) {
        const V a = sp[i], b = sp[i + 64], c = sp[i + 128], e = sp[i + 192];
        put<V, NT>(dp + i, a);
        put<V, NT>(dp + i + 64, b);
        put<V, NT>(dp + i + 128, c);
        put<V, NT>(dp + i + 192, e);
    }
    for (; i < n; i += 64) put<V, NT>(dp + i, sp[i]);
}

// bytes [0, n) of a segment whose source and destination addresses agree modulo sizeof(V): 2-byte elements up to the first
// V-aligned destination byte, whole V units, 2-byte elements behind the last
template <typename V, bool NT>
__device__ __forceinline__ void copy_aligned(const unsigned char* __restrict__ s, unsigned char* __restrict__ d, uint64_t n, uint32_t lane) {
    constexpr uint64_t W = sizeof(V);
    uint64_t head = (W - (reinterpret_cast<uintptr_t>(d) & (W - 1))) & (W - 1);
    if (head > n) head = n;
    const uint64_t units = (n - head) / W, tail = n - head - units * W;
    if (lane < head / 2) reinterpret_cast<unsigned short*>(d)[lane] = reinterpret_cast<const unsigned short*>(s)[lane];
    copy_units<V, NT>(s + head, d + head, units, lane);
    const uint64_t t0 = head + units * W;
    if (lane < tail / 2) reinterpret_cast<unsigned short*>(d + t0)[lane] = reinterpret_cast<const unsigned short*>(s + t0)[lane];
}

template <bool NT>
__global__ __launch_bounds__(256) void compact_runs_kernel(CompactArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    uint64_t pos = a.dst_begin + wave * kCompactWaveBytes;
    if (pos >= a.dst_end) return;
    const uint64_t end = pos + kCompactWaveBytes < a.dst_end ? pos + kCompactWaveBytes : a.dst_end;
    // the run `pos` lies in: the last one that begins at or before it (runs[0].dst = 0, runs[nruns].dst = the slab's size > pos)
    uint64_t lo = 0, hi = a.nruns;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a.runs[mid].dst <= pos) lo = mid;
        else hi = mid;
    }
    uint64_t run = lo;
    while (pos < end && run < a.nruns) {
        const CompactRun r = a.runs[run];
        const uint64_t run_end = a.runs[run + 1].dst;
        const uint64_t seg_end = run_end < end ? run_end : end;
        if (seg_end > pos) {   // (a plan never holds an empty run; one would only be stepped over)
            const unsigned char* base = (r.src & kCompactFromWal) ? a.wal : a.slab;
            const unsigned char* s = base + (r.src & ~kCompactFromWal) + (pos - r.dst);
            unsigned char* d = a.out + pos;
            const uint64_t n = seg_end - pos;
            const uintptr_t skew = reinterpret_cast<uintptr_t>(s) ^ reinterpret_cast<uintptr_t>(d);
            if ((skew & 15) == 0) copy_aligned<cu32x4, NT>(s, d, n, lane);
            else if ((skew & 7) == 0) copy_aligned<cu32x2, NT>(s, d, n, lane);
            else if ((skew & 3) == 0) copy_aligned<uint32_t, NT>(s, d, n, lane);
            else copy_units<unsigned short, NT>(s, d, n / 2, lane);
            pos = seg_end;
        }
        if (pos == run_end) ++run;
    }
}

}  // namespace

hipError_t launch_compact_runs(const CompactArgs& a, bool nt_stores, hipStream_t stream) {
    if (a.dst_end <= a.dst_begin || a.nruns == 0) return hipSuccess;
    const uint64_t waves = (a.dst_end - a.dst_begin + kCompactWaveBytes - 1) / kCompactWaveBytes;
    const uint64_t blocks = (waves + 3) / 4;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    if (nt_stores) hipLaunchKernelGGL(compact_runs_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(compact_runs_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace fsgpu
