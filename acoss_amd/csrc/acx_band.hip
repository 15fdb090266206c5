// libacx: launcher of the Serra09 band kernels (serra09_kernels.hpp, serra09_band2_kernels.hpp, K1').  A translation unit of
// its own: the Makefile compiles it with -mllvm -amdgpu-sched-strategy=max-ilp, which gives these kernels
// +1 % and would cost simple_kernel 26 % and ef_rowstat_kernel 20 %.
// WHICH kernel a pass runs is not decided here: serra09_plan.hpp holds the size classes, the kernel per class and the
// ACX_BAND2 switch; the launcher receives the family and maps it onto the instantiations.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cassert>

#include "serra09_kernels.hpp"
#include "serra09_band2_kernels.hpp"
#include "serra09_plan.hpp"

namespace acx {

namespace {

std::atomic<long long> g_fast_tail_launches{0};      // band passes of this process that took the FAST copy (fast_tail_launches)
std::atomic<long long> g_plane_launches{0};          // ... that read their column operands from the per-rotation planes (plane_launches)

// `family`: the plan's answer for the pass's size class (serra09_band_family, serra09_plan.hpp -- the class limits, the choice
// per stack size and arithmetic, and ACX_BAND2 live there); this switch only maps it onto the instantiations.
template <int M>
bool launch_band_m(const BandLaunch &L, const PairDesc *dpd, int B, int maxRows, int family, int role, int write_d2, int want_eps, int arith)
{
    const dim3 grid((maxRows + BAND - 1) / BAND, B, 1);
#define ACX_BAND_KP(V4_, R_, W_, A_, F_, P_) hipLaunchKernelGGL((band_kernel<M, V4_, R_, W_, A_, F_, P_>), grid, dim3(BAND_THREADS), 0, L.stream, \
                                                  L.frot, L.toff, L.normtab, L.noff, dpd, L.scratch, L.thr, L.bits, L.kappa, \
                                                  L.pct_mode, L.inclusive, L.oti_target, want_eps, L.planes, L.plane_floats)
    // the wide class of the exact arithmetic takes its column operands from the per-rotation planes when the context built them
#define ACX_BAND_K(V4_, R_, W_, A_, F_) do { if constexpr (V4_ == 8 && A_ == 0) { \
                                                 if (L.planes) { ACX_BAND_KP(V4_, R_, W_, A_, F_, true); g_plane_launches.fetch_add(1, std::memory_order_relaxed); } \
                                                 else ACX_BAND_KP(V4_, R_, W_, A_, F_, false); } \
                                             else ACX_BAND_KP(V4_, R_, W_, A_, F_, false); } while (0)
    // (the variant that also writes D2 exists for the row pass only: the debug entry point)
#define ACX_BAND_A(V4_, A_) do { if (role) ACX_BAND_K(V4_, 1, false, A_, false); else if (write_d2) ACX_BAND_K(V4_, 0, true, A_, false); else ACX_BAND_K(V4_, 0, false, A_, false); } while (0)
    // the product-path tail (band_row_tail's FAST copy): the plan found its conditions to hold for the pass and for every pair of the
    // launch (serra09_fast_tail_runs, serra09_plan.hpp: wide class, exact arithmetic, no D2, no eps, a bitmap in the row pass)
    if (L.fast_tail) {
        assert(family == ACX_SERRA09_FAMILY_BAND_8 && arith == ACX_ARITH_EXACT && !write_d2 && !want_eps);    // (serra09_fast_tail_params)
        if (role) ACX_BAND_K(8, 1, false, 0, true); else ACX_BAND_K(8, 0, false, 0, true);
        g_fast_tail_launches.fetch_add(1, std::memory_order_relaxed);
        return true;
    }
    // the opt-in f16x2 Gram: the default stack size only
#define ACX_BAND(V4_) do { if (arith == ACX_ARITH_EXACT) ACX_BAND_A(V4_, 0); else if constexpr (M == 9) ACX_BAND_A(V4_, 1); else return false; return true; } while (0)
    // the kernels of two and four rows per wave (serra09_band2_kernels.hpp): m <= 9, the exact arithmetic
#define ACX_BAND2_K(R_, W_, NV_, GL_) hipLaunchKernelGGL((band2_kernel<M, R_, W_, NV_, GL_>), grid, dim3(64 * B2Geom<NV_, GL_>::WAVES), 0, L.stream, L.frot, L.normtab, \
                                                         dpd, L.scratch, L.thr, L.bits, L.pct_mode, L.inclusive, L.oti_target, want_eps)
#define ACX_BAND2(NV_, GL_) do { if constexpr (M <= 9) { if (arith != ACX_ARITH_EXACT) return false; \
                                     if (role) ACX_BAND2_K(1, false, NV_, GL_); else if (write_d2) ACX_BAND2_K(0, true, NV_, GL_); else ACX_BAND2_K(0, false, NV_, GL_); \
                                     return true; } return false; } while (0)
    if (arith != ACX_ARITH_EXACT && arith != ACX_ARITH_F16X2) return false;
    switch (family) {
    case ACX_SERRA09_FAMILY_BAND2_4ROWS: ACX_BAND2(B2_NV, 16);
    case ACX_SERRA09_FAMILY_BAND2_2ROWS: ACX_BAND2(B2_NV, 32);
    case ACX_SERRA09_FAMILY_BAND2_MID: ACX_BAND2(B2_NV_MID, 32);
    case ACX_SERRA09_FAMILY_BAND_2: ACX_BAND(2);
    case ACX_SERRA09_FAMILY_BAND_4: ACX_BAND(4);
    case ACX_SERRA09_FAMILY_BAND_8: ACX_BAND(8);
    }
    return false;
#undef ACX_BAND2
#undef ACX_BAND2_K
#undef ACX_BAND
#undef ACX_BAND_A
#undef ACX_BAND_K
#undef ACX_BAND_KP
}

}  // namespace

bool launch_band_kernel(const BandLaunch &L, int m, const PairDesc *dpd, int B, int maxRows, int family, int role, int write_d2, int want_eps, int arith)
{
    switch (m) {
#define ACX_CASE(M_) case M_: return launch_band_m<M_>(L, dpd, B, maxRows, family, role, write_d2, want_eps, arith);
#ifdef ACX_FAST_BUILD   /* development builds: only the default stack size */
#ifndef ACX_FAST_BUILD_M
#define ACX_FAST_BUILD_M 9
#endif
        ACX_CASE(ACX_FAST_BUILD_M)
#else
        ACX_CASE(1) ACX_CASE(2) ACX_CASE(3) ACX_CASE(4) ACX_CASE(5) ACX_CASE(6) ACX_CASE(7) ACX_CASE(8)
        ACX_CASE(9) ACX_CASE(10) ACX_CASE(11) ACX_CASE(12) ACX_CASE(13) ACX_CASE(14) ACX_CASE(15) ACX_CASE(16)
#endif
#undef ACX_CASE
    }
    return false;
}

long long fast_tail_launches() { return g_fast_tail_launches.load(std::memory_order_relaxed); }
long long plane_launches() { return g_plane_launches.load(std::memory_order_relaxed); }

}  // namespace acx

#ifdef ACX_TIMING
// development builds: per-phase clock totals of band_kernel (slots 0-7; slot 15 = waves); reset != 0 clears them
extern "C" int acx_dev_band_timing(unsigned long long *out, int reset)
{
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(acx::g_band_clk), sizeof(unsigned long long) * 32) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[32] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(acx::g_band_clk), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif
