// GCM_PE25D, the zonal wavenumber spectra (gcm_set_spectra, gcm_spectra_sample, gcm_get_spectra): one launch per sample
// reads the current state once, transforms four real rows per (level, row) along i in float64 and adds the six raw
// products of the lowest M = mmax + 1 wavenumbers to float64 sums that live in the handle.  The contract and the word
// table: include/gcmcore.h.
//
//   per cell (float64, the storage type widened exactly, every product and sum rounded on its own):
//     uc = 0.5 (u[i] + u[i - 1]), i periodic;   vc = 0.5 (v[j] + v[j - 1]);   theta;   T = theta exner(sig[k] p + ptop)
//     row -1: row H - 1 on a single domain, a band's first north ghost row of v (as in pe25d_climate.hip)
//   per level two complex transforms of length W in LDS (fft_lds.h, forward, double2): z1 = uc + i vc, z2 = T + i theta;
//   the packed real rows come apart as X_m = (Z_m + conj Z_{W-m}) / 2, Y_m = (Z_m - conj Z_{W-m}) / (2i), index W - m at
//   m = 0 taken as 0, for m <= mmax only
//   words: |Uc|^2, |Vc|^2, |That|^2, Re(Uc conj Vc), Re(Vc conj That), Re(Vc conj Thetahat)
//
// Contraction is off for the whole file (the Makefile builds it with -ffp-contract=fast-honor-pragmas).
//
// The transform is the generic mixed-radix Stockham path of fft_lds.h for every width: the plan, the pass order and the
// workgroup size (512) are functions of W alone, so what a row contributes depends on the row's data, W and mmax only.
// Thread t owns the wavenumbers m = t, t + 512, ...: it keeps Uc_m and Vc_m in registers across the second transform
// (NM = 4 of them, which hold the 2023 wavenumbers of the widest row the LDS takes and stay within the 128 vector
// registers that let four waves share a SIMD), forms the six
// products and adds each to its accumulator word -- one writer per word and launch, no atomics, a run of M consecutive
// doubles per word and workgroup.  The state's layout is [j][k][i]; a workgroup walks a segment of the levels of its
// row j with p of the row widened and parked in LDS (a lane reads back only what it wrote) beside the Exner table.
//
// LDS of a launch: two double2 rows of W (the Stockham ping-pong), p of the row, the Exner table:
// 32 W + 8 (W rounded up to even) + 2048 bytes -- 59648 at W = 1440; above 64 KB the kernel's attribute is raised at
// registration, and what exceeds a workgroup's 160 KB is refused there (W > 4044).
#pragma clang fp contract(off)
#include "pe25d_host.h"

#include "pe25d_spectra.h"

namespace gcm {

static size_t sp_prow_doubles(int W) { return ((size_t)W + 1) & ~(size_t)1; }   // (the double2 rows behind it stay 16-byte aligned)
size_t spectra_lds_bytes(int W) { return sizeof(double) * (kExnerTabDoubles + sp_prow_doubles(W)) + 2 * sizeof(double2) * (size_t)W; }

int spectra_nseg(int H, int L, int cus) { return (int)std::min<long>(L, std::max<long>(1, (4L * cus + H - 1) / H)); }

void spectra_twiddles(int W, double2 *tw) {
    // 2 pi n / W = oct (pi / 4) + theta: 8 n = oct W + rem in integers, theta = pi rem / (4 W) in [0, pi / 4), an odd
    // octant mirrored (theta = pi (W - rem) / (4 W)); libm sees first-octant angles only, the axes come out exact
    for (int n = 0; n < W; ++n) {
        const long n8 = 8L * n;
        const int oct = (int)(n8 / W);
        long rem = n8 - (long)oct * W;
        if (oct & 1) rem = W - rem;
        const double th = M_PI * (double)rem / (4.0 * (double)W);
        const double c = std::cos(th), s = std::sin(th);
        double cr, sr;
        switch (oct) {
        case 0: cr = c; sr = s; break;
        case 1: cr = s; sr = c; break;
        case 2: cr = -s; sr = c; break;
        case 3: cr = -c; sr = s; break;
        case 4: cr = -c; sr = -s; break;
        case 5: cr = -s; sr = -c; break;
        case 6: cr = s; sr = -c; break;
        default: cr = c; sr = -s; break;
        }
        tw[n].x = cr;
        tw[n].y = -sr;
    }
}

// the two real rows packed in z, at wavenumber m: X_m and Y_m
__device__ __forceinline__ void sp_unpack(const double2 *z, int m, int W, double2 &X, double2 &Y) {
    const double2 a = z[m], b = z[m == 0 ? 0 : W - m];
    X.x = 0.5 * (a.x + b.x);
    X.y = 0.5 * (a.y - b.y);
    Y.x = 0.5 * (a.y + b.y);
    Y.y = -0.5 * (a.x - b.x);
}

// grid (rows, level segments).  Every thread reaches every barrier: the loops over i and m are guarded, not left
template <typename T, int NM>
__global__ __launch_bounds__(kSpThreads) void pe_spectra_kernel(SpectraArgs a) {
    extern __shared__ __align__(16) double sp_lds[];
    const int W = a.W, L = a.L, H = a.H, M = a.M;
    double *tab = sp_lds, *prow = tab + kExnerTabDoubles;
    double2 *x = (double2 *)(prow + (((size_t)W + 1) & ~(size_t)1)), *y = x + W;
    for (int n = threadIdx.x; n < kExnerTabDoubles; n += kSpThreads) tab[n] = a.exner_tab[n];
    const int j = (int)blockIdx.x, seg = (int)blockIdx.y;
    const int t0 = (int)threadIdx.x;
    const int k0 = (int)((long)seg * L / a.nseg), k1 = (int)((long)(seg + 1) * L / a.nseg);
    const int jm = (a.wrap && j == 0) ? H - 1 : j - 1;
    const T *pj = (const T *)a.p + (long)j * W;
    for (int i = t0; i < W; i += kSpThreads) prow[i] = (double)pj[i];
    __syncthreads();
    for (int k = k0; k < k1; ++k) {
        double2 U[NM], V[NM];
#pragma unroll
        for (int q = 0; q < NM; ++q) U[q] = V[q] = double2{0.0, 0.0};
        // the two transforms of the level take one pass of this loop each: fft_lds then has one call site and is compiled
        // into the kernel (called from two it stayed a function, with a stack frame in scratch)
#pragma clang loop unroll(disable)
        for (int half = 0; half < 2; ++half) {
            // (the level as each part of the pass sees it, opaque to the optimiser: the rows' addresses and the level's
            // constants are then formed where they are used and do not occupy scalar registers across the transform)
            int kk = k;
            asm volatile("" : "+s"(kk));
            if (half == 0) {                                   // z1 = uc + i vc
                const T *ur = (const T *)a.u + ((long)j * L + kk) * W;
                const T *vr = (const T *)a.v + ((long)j * L + kk) * W;
                const T *vn = (const T *)a.v + ((long)jm * L + kk) * W;
                for (int ib = t0; ib < W; ib += kSpBatch * kSpThreads) {
                    T xu[kSpBatch], xw[kSpBatch], xv[kSpBatch], xn[kSpBatch];
#pragma unroll
                    for (int b = 0; b < kSpBatch; ++b) {
                        const int i = ib + b * kSpThreads;
                        if (i >= W) break;
                        xu[b] = ur[i];
                        xw[b] = ur[i == 0 ? W - 1 : i - 1];
                        xv[b] = vr[i];
                        xn[b] = vn[i];
                    }
#pragma unroll
                    for (int b = 0; b < kSpBatch; ++b) {
                        const int i = ib + b * kSpThreads;
                        if (i >= W) break;
                        double2 z;
                        z.x = 0.5 * ((double)xu[b] + (double)xw[b]);
                        z.y = 0.5 * ((double)xv[b] + (double)xn[b]);
                        x[i] = z;
                    }
                }
            } else {                                           // z2 = T + i theta
                const T *tr = (const T *)a.t + ((long)j * L + kk) * W;
                const double sg = a.sig[kk];
                for (int ib = t0; ib < W; ib += kSpBatch * kSpThreads) {
                    T xt[kSpBatch];
#pragma unroll
                    for (int b = 0; b < kSpBatch; ++b) {
                        const int i = ib + b * kSpThreads;
                        if (i >= W) break;
                        xt[b] = tr[i];
                    }
#pragma unroll
                    for (int b = 0; b < kSpBatch; ++b) {
                        const int i = ib + b * kSpThreads;
                        if (i >= W) break;
                        const double th = (double)xt[b];
                        const double pl = sg * prow[i] + a.ptop;
                        double2 z;
                        z.x = th * exner(pl, tab);
                        z.y = th;
                        x[i] = z;
                    }
                }
            }
            __syncthreads();
            const double2 *z = fft_lds<false>(x, y, a.tw, a.plan);
            if (half == 0) {
#pragma unroll
                for (int q = 0; q < NM; ++q) {
                    const int m = t0 + q * kSpThreads;
                    if (m < M) sp_unpack(z, m, W, U[q], V[q]);
                }
            } else {
                int kp = k;
                asm volatile("" : "+s"(kp));
                const long word = (long)L * H * M;
                double *sk = a.s + ((long)kp * H + j) * M;
#pragma unroll
                for (int q = 0; q < NM; ++q) {
                    const int m = t0 + q * kSpThreads;
                    if (m < M) {
                        double2 Tm, Th;
                        sp_unpack(z, m, W, Tm, Th);
                        const double2 Um = U[q], Vm = V[q];
                        sk[m] += Um.x * Um.x + Um.y * Um.y;
                        sk[word + m] += Vm.x * Vm.x + Vm.y * Vm.y;
                        sk[2 * word + m] += Tm.x * Tm.x + Tm.y * Tm.y;
                        sk[3 * word + m] += Um.x * Vm.x + Um.y * Vm.y;
                        sk[4 * word + m] += Vm.x * Tm.x + Vm.y * Tm.y;
                        sk[5 * word + m] += Vm.x * Th.x + Vm.y * Th.y;
                    }
                }
            }
            __syncthreads();                                   // (everybody has read z before x is packed again)
        }
    }
}

// the instantiation that holds M wavenumbers in the workgroup's threads, nullptr beyond kSpMaxPerThread a thread
template <typename T>
static const void *sp_kernel_for(int M) {
    const int per = (M + kSpThreads - 1) / kSpThreads;
    // (one instantiation: with 1, 2 or 3 a thread the compiler leaves some of the kernels an unused 36-byte stack slot
    // from its scalar spills, which would make every launch ask for scratch; 4 stay within the 128 vector registers of
    // four waves a SIMD, and the wavenumbers a thread does not own cost it a compare each)
    if (per <= kSpMaxPerThread) return (const void *)pe_spectra_kernel<T, kSpMaxPerThread>;
    return nullptr;
}
static const void *sp_kernel(const Pe25d *m, int M) { return m->f32 ? sp_kernel_for<float>(M) : sp_kernel_for<double>(M); }

// ---------------------------------------------------------------- the handle's side
// layout of the sampler's buf: tw [W] double2 | sig [L] | s [GCM_SPEC_WORDS][L][H][M].  every, due, reset, get, put and
// free are the samplers' shared routines (pe25d_sampler_*, pe25d_state.hip)

// A second registration with the same mmax zeroes the sums in place, with another it takes a new buffer
int pe25d_set_spectra(Pe25d *m, int every, int mmax, hipStream_t s, std::string *err) {
    PeSpectra &z = m->spec;
    if (every < 0) { *err = "gcm_set_spectra: every must be >= 0"; return GCM_ERR_ARG; }
    if (every == 0) {
        if (!z.buf) return GCM_OK;
        // (a sample may still be adding to the sums)
        if (int rc = hip_rc(hipStreamSynchronize(s), "gcm_set_spectra", err)) return rc;
        pe25d_sampler_free(m, kSampleSpectra);
        return GCM_OK;
    }
    if (mmax < -1 || mmax > m->W / 2) {
        *err = "gcm_set_spectra: mmax must be -1 (the default) or within 0 .. W / 2 = " + std::to_string(m->W / 2);
        return GCM_ERR_ARG;
    }
    if (mmax < 0) mmax = std::min(m->W / 2, 63);
    const int M = mmax + 1;
    const size_t lds = spectra_lds_bytes(m->W);
    const void *kern = sp_kernel(m, M);
    if (lds > kSpLdsCap || !kern || m->plan.n != m->W) {
        *err = "gcm_set_spectra: the transform buffers of a row of " + std::to_string(m->W) + " columns take " + std::to_string(lds) +
               " bytes of LDS, a workgroup has " + std::to_string(kSpLdsCap);
        return GCM_ERR_UNSUPPORTED;
    }
    if (int rc = hip_rc(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "gcm_set_spectra", err)) return rc;
    const size_t head = 2 * (size_t)m->W + m->L, sums = (size_t)GCM_SPEC_WORDS * m->L * m->H * M;
    if (z.buf && z.mmax == mmax) {
        if (int rc = hip_rc(hipMemsetAsync(z.buf + head, 0, sizeof(double) * sums, s), "gcm_set_spectra", err)) return rc;
    } else {
        if (z.buf) {
            if (int rc = hip_rc(hipStreamSynchronize(s), "gcm_set_spectra", err)) return rc;
            pe25d_sampler_free(m, kSampleSpectra);
        }
        std::vector<double> init(head + sums, 0.0);
        spectra_twiddles(m->W, (double2 *)init.data());
        std::copy(m->sig_host.begin(), m->sig_host.end(), init.begin() + 2 * (size_t)m->W);
        if (!dev_upload<double>(m, &z.buf, init.data(), init.size())) {
            // (dev_upload keeps what it allocated in the handle's list: gcm_destroy frees it)
            z = PeSpectra{};
            *err = "hip: gcm_set_spectra allocation failed";
            return GCM_ERR_HIP;
        }
    }
    z.head = head;
    z.words[0] = sums;
    z.words[1] = 0;
    z.every = every;
    z.mmax = mmax;
    z.steps = 0;
    z.n = 0;
    return GCM_OK;
}

int pe25d_spectra_mmax(const Pe25d *m) { return m->spec.mmax; }

// The launch reads p, u, v and theta of the current state set, and on a band v's first north ghost row, like the
// climatology's; how it is ordered against the stages that follow: pe25d_kernels.h, at the samplers' declarations
int pe25d_spectra_sample(Pe25d *m, hipStream_t s, std::string *err) {
    if (int rc = pe25d_sampler_registered(m, kSampleSpectra, "gcm_spectra_sample", err)) return rc;
    PeSpectra &z = m->spec;
    const int set = m->cur_i;
    SpectraArgs a{};
    a.p = state_field(m, set, GCM_P); a.u = state_field(m, set, GCM_U);
    a.v = state_field(m, set, GCM_V); a.t = state_field(m, set, GCM_T);
    a.tw = (const double2 *)z.buf; a.sig = z.buf + 2 * (size_t)m->W; a.exner_tab = m->exner_tab;
    a.s = z.buf + z.head;
    a.ptop = m->cfg.ptop;
    a.plan = m->plan;
    a.W = m->W; a.H = m->H; a.L = m->L; a.M = z.mmax + 1; a.wrap = m->wrap ? 1 : 0;
    a.nseg = spectra_nseg(a.H, a.L, m->cus);
    void *args[] = {&a};
    const hipError_t e = hipLaunchKernel(sp_kernel(m, a.M), dim3((unsigned)a.H, (unsigned)a.nseg), dim3(kSpThreads), args,
                                         spectra_lds_bytes(a.W), s);
    if (int rc = hip_rc(e, "gcm_spectra_sample", err)) return rc;
    ++z.n;
    return GCM_OK;
}

int pe25d_spectra_plan(const Pe25d *m, int *out, int nout) {
    if (!out || nout < GCM_SPEC_PLAN_WORDS) return GCM_ERR_ARG;
    const int M = m->spec.every > 0 ? m->spec.mmax + 1 : std::min(m->W / 2, 63) + 1;
    out[0] = m->H;
    out[1] = spectra_nseg(m->H, m->L, m->cus);
    out[2] = kSpThreads;
    out[3] = (int)spectra_lds_bytes(m->W);
    out[4] = m->plan.nrad;
    out[5] = (M + kSpThreads - 1) / kSpThreads;
    return GCM_OK;
}

}  // namespace gcm
