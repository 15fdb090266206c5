// SiMPle: the matrix profile, its index and the matched section of an ordered pair.
//
// simple_kernel (simple_kernels.hpp) computes every profile value MP[a] = min_b D[a, b], takes the median and throws the rest
// away.  simple_profile_kernel is its second edition for the callers that ask WHERE: the same distances by the same operations
// in the same order (window norms of simple_winnorm_kernel, row 0 and column 0 in full, dot = (prev - gold) + gnew down the
// diagonals, fma(-2, dot, a2 + w)) -- so -median(MP) has the bits simple_kernel returns --, and beside the running minimum of
// every lane the COLUMN at which it was first attained:
//   MPI[a]   the smallest b with D[a, b] == MP[a]: the sweep walks the columns upwards and replaces the index on a strict `<`
//            only; row 0, whose columns are strided over the lanes, is reduced across the lanes by (value, column);
//   best     best_q = the smallest a with MP[a] == min MP, best_r = MPI[best_q], best_dist = MP[best_q];
//   section  the longest maximal run of rows a0 .. a0 + n - 1 with MPI[a + 1] == MPI[a] + 1 (a diagonal of the distance matrix:
//            n consecutive subsequences of the query whose nearest neighbours are consecutive in the reference); of several
//            longest the one with the smallest a0.
// One WAVE per ordered pair and no workgroup barrier, the sweep, the row groups with their feeder lanes, the E hand-over through
// LDS and the median by ballot search are simple_kernel's; f64_key / key_f64 / simple_select_key and the window norms are
// shared with it, not copied.  The index costs the sweep one v_cmp_lt_f64 and ONE 32-bit select per step (the value stays one
// v_min_f64): no two selects on vcc stand next to each other (profiles/r06_cndmask_probe.txt).
// LDS per pair: simple_kernel's 8 (nb + na + row groups) bytes + 4 ma for the index.
#pragma once
#include "simple_kernels.hpp"

namespace acx {

// What the kernel leaves per pair (the layout of acx_simple_alignment, include/acx.h: the driver asserts it)
struct SimpleProfileRec {
    double score, best_dist;
    int32_t shift, best_q, best_r, q0, r0, q1, r1, q_span[2], r_span[2], run_len;
};
static_assert(sizeof(SimpleProfileRec) == 64, "two doubles and twelve int32");

// Waves per SIMD the kernel is compiled for, from the compiler's resource report for gfx950: the index
// and the step of the round are two registers more than simple_kernel holds at seven waves, where every L from 3 on spills.  Six
// waves (80 registers) hold L <= 8 without a spill, L = 9 and 10 (rounds of 18 and 10 steps) need five (96 registers: 89 and 81
// used); from L = 11 on the compiler chooses, as for simple_kernel.  -DACX_SIMPLE_PROFILE_WAVES=N overrides (A/B builds).
#ifdef ACX_SIMPLE_PROFILE_WAVES
constexpr int simple_profile_waves(int) { return ACX_SIMPLE_PROFILE_WAVES; }
#else
constexpr int simple_profile_waves(int l) { return l <= 8 ? 6 : l <= 10 ? 5 : 1; }
#endif

template <int L>
__global__ __launch_bounds__(64 * SIMPLE_WPB, simple_profile_waves(L)) void simple_profile_kernel(
    const double *__restrict__ pool, const int64_t *__restrict__ toff, const double *__restrict__ prof,
    const double *__restrict__ wn, const int32_t *__restrict__ pairs, SimpleProfileRec *__restrict__ out,
    const int64_t *__restrict__ poff,          // where pair p's profile starts in out_mp / out_mpi; nullptr: the records alone
    double *__restrict__ out_mp, int32_t *__restrict__ out_mpi, int do_oti, int npairs, int smem_per_wave)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_all[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pidx = blockIdx.x * (int)(blockDim.x >> 6) + wave;
    if (pidx >= npairs) return;                                  // wave-uniform
    unsigned char *smem_raw = smem_all + (size_t)wave * smem_per_wave;
    const int ti = pairs[2 * pidx], tj = pairs[2 * pidx + 1];
    const int64_t oa = toff[ti], ob = toff[tj];
    const int na = (int)(toff[ti + 1] - oa), nb = (int)(toff[tj + 1] - ob);
    const int ma = na - L + 1, mb = nb - L + 1;
    // E as in simple_kernel (one array, every group stores one slot below the one it has just read), then the keys of the
    // profile, then its index
    constexpr int STRIDE = 64 - L;
    static_assert(L >= 1 && L <= 16, "feeder lanes");
    const int ngroups_ = (ma + STRIDE - 1) / STRIDE;
    double *E = reinterpret_cast<double *>(smem_raw);            // mb + ngroups_ + 1 slots
    unsigned long long *mp = reinterpret_cast<unsigned long long *>(E + mb + ngroups_ + 1);   // ma keys
    int32_t *mpi = reinterpret_cast<int32_t *>(mp + ma);          // ma columns

    // ---- OTI: simple_kernel's (ties: the highest shift)
    int shift = 0;
    if (do_oti) {
        const double *pa = prof + (size_t)ti * 12, *pb = prof + (size_t)tj * 12;
        double bestv = 0.0;
        for (int s = 0; s < 12; ++s) {
            double acc = 0.0;
            for (int c = 0; c < 12; ++c) acc += pa[c] * pb[(c - s + 12) % 12];
            if (s == 0 || acc >= bestv) { bestv = acc; shift = s; }
        }
    }
    const double *ga = pool + oa * 12, *gb = pool + ob * 12;
    const double *wa = wn + oa, *wb = wn + ob;
    auto load_a = [&](int t, double (&v)[12]) {
#pragma unroll
        for (int c = 0; c < 12; ++c) {
            int cs = c + shift; if (cs >= 12) cs -= 12;
            v[c] = ga[(size_t)t * 12 + cs];
        }
    };
    auto dot12 = [&](const double (&a)[12], const double *brow) {
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < 12; ++c) acc = __builtin_fma(a[c], brow[c], acc);
        return acc;
    };

    // ---- row 0 in full (lanes over b).  A lane meets its columns in rising order and keeps the first of equal values; across
    // the lanes the order is (value, column): the first minimum of the row, whichever lane and whichever 64-stride holds it
    {
        unsigned long long k0 = 0xffffffffffffffffull;
        int c0 = 0x7fffffff;
        const double a2_0 = wa[0];
        for (int b = lane; b < mb; b += 64) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < L; ++k) {
                double ak[12];
                load_a(k, ak);
                acc += dot12(ak, gb + (size_t)(b + k) * 12);
            }
            E[b + ngroups_] = acc;
            const unsigned long long kd = f64_key((a2_0 + wb[b]) - 2.0 * acc);
            if (kd < k0) { k0 = kd; c0 = b; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long ok = __shfl_xor(k0, o);
            const int oc = __shfl_xor(c0, o);
            if (ok < k0 || (ok == k0 && oc < c0)) { k0 = ok; c0 = oc; }
        }
        if (lane == 0) { mp[0] = k0; mpi[0] = c0; }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();

    // ---- the row groups: simple_kernel's sweep (its comments there), with the column of the running minimum beside it
    const int ngroups = (ma - 1 + STRIDE - 1) / STRIDE;             // rows 1 .. ma - 1
    const int vl = (lane + L) & 63;
    const int up_src = ((lane - L) & 63) << 2;
    auto shift_up_L = [&](double v) {
        const long long bits = __double_as_longlong(v);
        const int lo = __builtin_amdgcn_ds_bpermute(up_src, (int)(bits & 0xffffffffll));
        const int hi = __builtin_amdgcn_ds_bpermute(up_src, (int)(bits >> 32));
        return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
    };
    for (int g = 0; g < ngroups; ++g) {
        const int a = STRIDE * g + 1 + vl - L;
        const bool valid = vl >= L && a < ma;
        const int ac = a < 0 ? 0 : (a > ma - 1 ? ma - 1 : a);
        int fa = a + L - 1;
        fa = fa < 0 ? 0 : (fa > na - 1 ? na - 1 : fa);
        const int eoff = ngroups_ - g;
        const bool more = g + 1 < ngroups;
        double An[12];
        load_a(fa, An);
        const double a2 = wa[ac];
        double dot = 0.0;
        {
#pragma unroll
            for (int k = 0; k < L; ++k) {
                double ak[12];
                load_a(ac + k, ak);
                dot += dot12(ak, gb + (size_t)k * 12);
            }
        }
        double mn = (a2 + wb[0]) - 2.0 * dot;
        int mi = 0;                                             // column 0 holds the minimum until a later one is SMALLER
        if (more && vl == 63) E[eoff - 1] = dot;
        double ring[L];
#pragma unroll
        for (int j = 0; j < L; ++j) ring[(1 + j) % L] = shift_up_L(dot12(An, gb + (size_t)j * 12));
        double bn[2][12];
#pragma unroll
        for (int q = 0; q < 2; ++q)
            if (1 + q < mb) {
                const double *pn = gb + (size_t)(L + q) * 12;
#pragma unroll
                for (int c = 0; c < 12; ++c) bn[(1 + q) & 1][c] = pn[c];
            }
        constexpr int UN = (L % 2 == 0) ? L : 2 * L;
        typedef __attribute__((address_space(3))) double lds_f64;
        typedef __attribute__((address_space(3))) void lds_void_;
        double w2[2] = {0.0, 0.0};
        static_assert(UN % 2 == 0, "window norms in pairs");
        auto round = [&](int b0, auto full_tag) {
            constexpr bool FULL = decltype(full_tag)::value;
            unsigned rbase = (unsigned)(uintptr_t)(lds_void_ *)(E + (b0 - 1 + eoff));
            asm volatile("" : "+v"(rbase));
            // the step of this round that lowered the minimum last (-1: none).  The step number is an immediate of the select; the
            // column b0 + j itself, a scalar beside vcc, would first have to be moved into a vector register for every step -- and
            // the compiler moves all UN of them ahead of the round (up to 30 registers: the ring spilled).  Once per round the step
            // becomes a column
            int loc = -1;
#pragma unroll
            for (int j = 0; j < UN; ++j) {
                const int b = b0 + j;
                if (FULL || b < mb) {                               // wave-uniform
                    if (L >= 2 ? j % 2 == 0 : true) { w2[j % 2] = wb[b]; if (L >= 2) w2[1] = wb[b + 1]; }
                    const double w = w2[j % 2];
                    const double e = *(const lds_f64 *)(rbase + 8u * j);
                    double prev;
                    {
                        const long long bits_ = __double_as_longlong(dot), ebits_ = __double_as_longlong(e);
                        const int lo_ = __builtin_amdgcn_update_dpp((int)(ebits_ & 0xffffffffll), (int)(bits_ & 0xffffffffll), 0x138, 0xf, 0xf, false);
                        const int hi_ = __builtin_amdgcn_update_dpp((int)(ebits_ >> 32), (int)(bits_ >> 32), 0x138, 0xf, 0xf, false);
                        prev = __longlong_as_double(((long long)hi_ << 32) | (unsigned int)lo_);
                    }
                    double gnew = 0.0;
#pragma unroll
                    for (int c = 0; c < 12; ++c) gnew = __builtin_fma(An[c], bn[(1 + j) & 1][c], gnew);
                    asm volatile("" : "+v"(gnew));
                    if (FULL || b + 2 < mb) {
                        const double *pn = gb + (size_t)(b + 1 + L) * 12;
#pragma unroll
                        for (int c = 0; c < 12; ++c) bn[(1 + j) & 1][c] = pn[c];
                    }
                    const double gold = ring[(1 + j) % L];
                    ring[(1 + j) % L] = shift_up_L(gnew);
                    dot = (prev - gold) + gnew;
                    const double dist = __builtin_fma(-2.0, dot, a2 + w);
                    // the index: one compare and ONE 32-bit select; the value stays simple_kernel's single v_min_f64.  Strict `<`: of
                    // equal distances the first column keeps the row
                    loc = dist < mn ? j : loc;
                    asm volatile("" : "+v"(loc));                   // the select stays in its step: left free, the compiler keeps the
                                                                    // round's UN compare masks and selects for later (the ring spilled)
                    asm("v_min_f64 %0, %1, %2" : "=v"(mn) : "v"(dist), "v"(mn));
                    if (more && vl == 63) *(lds_f64 *)(rbase + 8u * j) = dot;
                }
            }
            mi = loc >= 0 ? b0 + loc : mi;
        };
        int b0 = 1;
        for (; b0 + UN + 1 < mb; b0 += UN) round(b0, std::true_type());
        for (; b0 < mb; b0 += UN) round(b0, std::false_type());
        if (valid) { mp[a] = f64_key(mn); mpi[a] = mi; }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }

    // ---- the score: simple_kernel's median
    const int r_lo = (ma - 1) / 2, r_hi = ma / 2;
    const double vlo = key_f64(simple_select_key(mp, ma, r_lo, lane));
    const double vhi = (r_hi == r_lo) ? vlo : key_f64(simple_select_key(mp, ma, r_hi, lane));
    const double score = -((r_lo == r_hi) ? vlo : (vlo + vhi) * 0.5);

    // ---- best_q: the first row at which the profile is smallest.  One pass: a lane keeps the first of its rows' equal values,
    // the lanes are reduced by (value, row)
    unsigned long long bk = 0xffffffffffffffffull;
    int bq = 0x7fffffff;
    for (int i = lane; i < ma; i += 64) {
        const unsigned long long k = mp[i];
        if (k < bk) { bk = k; bq = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long ok = __shfl_xor(bk, o);
        const int oq = __shfl_xor(bq, o);
        if (ok < bk || (ok == bk && oq < bq)) { bk = ok; bq = oq; }
    }

    // ---- the longest run of MPI[a] == MPI[a - 1] + 1: a segmented scan over the BREAK flags (row 0, every row that does not
    // continue its predecessor's diagonal, and the row behind the last one), 64 rows per ballot.  The run that ends in front of
    // a break at row a started at the last break before it: the highest set bit below this lane in the chunk's ballot, or the
    // last break of the chunks before (`carry`, wave-uniform).  A lane keeps the longest run that its breaks close, the first of
    // equal lengths (its rows rise); the lanes are reduced by (length, smallest start).
    int blen = 0, bstart = 0x7fffffff, carry = 0;
    for (int i0 = 0; i0 <= ma; i0 += 64) {                          // wave-uniform trip count (row ma closes the last run)
        const int i = i0 + lane;
        const bool brk = i <= ma && (i == 0 || i == ma || mpi[i] != mpi[i - 1] + 1);
        const unsigned long long m = __ballot(brk);
        if (brk) {
            const unsigned long long below = m & ((1ull << lane) - 1ull);
            const int ps = below ? i0 + 63 - __clzll((long long)below) : carry;
            const int len = i - ps;
            if (len > blen) { blen = len; bstart = ps; }
        }
        if (m) carry = i0 + 63 - __clzll((long long)m);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int ol = __shfl_xor(blen, o), os = __shfl_xor(bstart, o);
        if (ol > blen || (ol == blen && os < bstart)) { blen = ol; bstart = os; }
    }

    if (lane == 0) {
        SimpleProfileRec r;
        r.score = score;
        r.best_dist = key_f64(bk);
        r.shift = shift;
        r.best_q = bq;
        r.best_r = mpi[bq];
        r.q0 = bstart;
        r.r0 = mpi[bstart];
        r.q1 = bstart + blen - 1;
        r.r1 = r.r0 + blen - 1;
        r.q_span[0] = r.q0; r.q_span[1] = r.q1 + L - 1;
        r.r_span[0] = r.r0; r.r_span[1] = r.r1 + L - 1;
        r.run_len = blen;
        out[pidx] = r;
    }
    if (poff) {
        const int64_t o = poff[pidx];
        for (int i = lane; i < ma; i += 64) {
            out_mp[o + i] = key_f64(mp[i]);
            out_mpi[o + i] = mpi[i];
        }
    }
}

}  // namespace acx
