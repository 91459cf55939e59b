// GCM_PE25D, the forcing of the passive tracers (gcm_set_tracer_forcing): source, emission, decay and pinned cells,
// one launch right behind each corrector launch of the tracer kernel, over the same rows, for the forced tracers only.
//
//   c1 = c + dt * (source + e);  c2 = c1 * fac;  c = pinned ? pin : c2
//
// Every operation is rounded on its own: contraction is off for the whole file (the Makefile builds it with
// -ffp-contract=fast-honor-pragmas), so a NumPy restatement in the handle's real type gives the same bits.
//
// A run of rows of one tracer is one contiguous run of elements (rows are L * W elements, [j][k][i]); the emission
// and the mask are stored in the same order, so the kernel is a 1-D march: 16 bytes of c per lane (2 doubles or 4
// floats), a wave's request one contiguous KiB.  A run need not start on 16 bytes (L * W = 30 in fp32, a band's ghost
// rows in front of own row 0): the elements up to the first boundary and behind the last whole vector are done one
// by one.  Addresses are a wave-uniform base (entry, run, pass) plus one 32-bit byte offset per
// lane, as in pe25d_tracer.h.  The fields a tracer did not register are never read: the branches are per entry,
// uniform for the workgroup.
#pragma clang fp contract(off)
#include <algorithm>
#include <cstdint>

#include "pe25d_tracer_force.h"
#include "pe25d_phase_geometry.h"

namespace gcm {

// (kTfThreads, kTfGroupsMax -- the most workgroups per entry: pe25d_phase_geometry.h)

template <typename T>
__device__ inline T tf_cell(T c, T e, bool pinned, T source, T dt, T fac, T pin) {
    const T se = source + e;
    const T d = dt * se;
    const T c1 = c + d;
    const T c2 = c1 * fac;
    return pinned ? pin : c2;
}

#define TF_GLOBAL __attribute__((address_space(1)))

// a wave-uniform address through an opaque scalar register pair (pe25d_tracer.h's sbase): the request is then the
// scalar base + the lane's 32-bit offset, not a 64-bit address per lane
__device__ inline TF_GLOBAL char *tf_sbase(const void *p) {
    unsigned long long v = (unsigned long long)p;
    unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
    lo = __builtin_amdgcn_readfirstlane(lo);
    hi = __builtin_amdgcn_readfirstlane(hi);
    asm volatile("" : "+s"(lo), "+s"(hi));
    return (TF_GLOBAL char *)(((unsigned long long)hi << 32) | lo);
}

// one element, `at` elements from own row 0
template <typename T>
__device__ inline void tf_one(const TracerForceEntryT<T> &en, long at, T dt) {
    TF_GLOBAL T *c = (TF_GLOBAL T *)en.c + at;
    const T e = en.emis ? ((const TF_GLOBAL T *)en.emis)[at] : T(0);
    const bool pinned = en.mask && ((const TF_GLOBAL unsigned char *)en.mask)[at] != 0;
    *c = tf_cell<T>(*c, e, pinned, en.source, dt, en.fac, en.pin);
}

// the whole vectors of a run: nvec of them from element `at0` on.  EM, MK: the entry has an emission / a mask (one
// straight-line body per combination, chosen per entry in tf_run)
template <typename T, bool EM, bool MK>
__device__ inline void tf_vectors(const TracerForceEntryT<T> &en, long at0, long nvec, T dt) {
    constexpr int V = 16 / (int)sizeof(T);
    typedef T vec_t __attribute__((ext_vector_type(V)));
    typedef unsigned char mvec_t __attribute__((ext_vector_type(V)));
    const unsigned item = (unsigned)blockIdx.x * kTfThreads + (unsigned)threadIdx.x;
    const long pass = (long)gridDim.x * kTfThreads;
    for (long b = 0; b < nvec; b += pass) {
        if (b + item >= nvec) break;
        const long at = at0 + b * V;                              // (wave-uniform)
        // (the lane offsets are made opaque once per pass, so that their widening stays next to the requests)
        unsigned ob = item * 16u, om = item * (unsigned)V;
        asm volatile("" : "+v"(ob), "+v"(om));
        const vec_t x = *(const TF_GLOBAL vec_t *)(tf_sbase(en.c + at) + ob);
        vec_t e = (vec_t)(T(0));
        if (EM) e = *(const TF_GLOBAL vec_t *)(tf_sbase(en.emis + at) + ob);
        mvec_t mk = (mvec_t)((unsigned char)0);
        if (MK) mk = *(const TF_GLOBAL mvec_t *)(tf_sbase(en.mask + at) + om);
        vec_t y;
#pragma unroll
        for (int v = 0; v < V; ++v) y[v] = tf_cell<T>(x[v], e[v], mk[v] != 0, en.source, dt, en.fac, en.pin);
        *(TF_GLOBAL vec_t *)(tf_sbase(en.c + at) + ob) = y;
    }
}

template <typename T>
__device__ inline void tf_run(const TracerForceEntryT<T> &en, long off, long n, T dt) {
    constexpr int V = 16 / (int)sizeof(T);
    if (n <= 0) return;
    const uintptr_t ca = (uintptr_t)(en.c + off);
    // the fields are placed like c (see TracerForceEntryT); if one is not, the whole run goes element by element
    const bool placed = (!en.emis || (((uintptr_t)(en.emis + off) ^ ca) & 15) == 0) &&
                        (!en.mask || (((uintptr_t)(en.mask + off) ^ (ca / sizeof(T))) & (V - 1)) == 0);
    const long head = placed ? std::min<long>(n, (long)((V - (ca / sizeof(T)) % V) % V)) : n;
    const long nvec = (n - head) / V;
    const long tail0 = head + nvec * V;
    if (en.emis) {
        if (en.mask) tf_vectors<T, true, true>(en, off + head, nvec, dt);
        else tf_vectors<T, true, false>(en, off + head, nvec, dt);
    } else {
        if (en.mask) tf_vectors<T, false, true>(en, off + head, nvec, dt);
        else tf_vectors<T, false, false>(en, off + head, nvec, dt);
    }
    // the elements in front of the first whole vector and behind the last, spread over the grid like the vectors
    // (placed: fewer than V each; else head == n: the whole run, one element per lane and pass)
    const long item = (long)blockIdx.x * kTfThreads + (long)threadIdx.x, pass = (long)gridDim.x * kTfThreads;
    for (long i = item; i < head; i += pass) tf_one<T>(en, off + i, dt);
    for (long i = tail0 + item; i < n; i += pass) tf_one<T>(en, off + i, dt);
}

// grid (workgroups, entries)
template <typename T>
__global__ __launch_bounds__(kTfThreads) void pe_tracer_force_kernel(TracerForceArgsT<T> a) {
    const TracerForceEntryT<T> &en = a.e[blockIdx.y];
    tf_run<T>(en, a.off0, a.n0, a.dt);
    tf_run<T>(en, a.off1, a.n1, a.dt);
}

template <typename T>
void launch_tracer_force(const TracerForceArgsT<T> &a, int entries, hipStream_t s) {
    const long n = std::max(a.n0, a.n1);
    if (entries <= 0 || n <= 0) return;
    const long groups = phase_tracer_force_groups(n, (int)sizeof(T));
    hipLaunchKernelGGL(pe_tracer_force_kernel<T>, dim3((unsigned)groups, (unsigned)entries), dim3(kTfThreads), 0, s, a);
}

template void launch_tracer_force<double>(const TracerForceArgsT<double> &, int, hipStream_t);
template void launch_tracer_force<float>(const TracerForceArgsT<float> &, int, hipStream_t);

}  // namespace gcm
