// libacx.so -- host side of the C ABI declared in include/acx.h.
//
// Owns the HIP device state (stream, packed feature pool in HBM, per-batch scratch arena)
// and drives the kernels of serra09_kernels.hpp over batches of track pairs.  No torch, no
// CPU fallback: if the device or a launch fails the call returns an error code.
#include <hip/hip_runtime.h>

#include <chrono>
#include <dlfcn.h>
#include <rccl/rccl.h>      // types and prototypes only: librccl is dlopen()ed when a communicator is asked for (acx_comm_init)

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <optional>
#include <string>
#include <vector>

#include "../../include/acx.h"
#include "serra09_kernels.hpp"
#include "serra09_long_kernels.hpp"
#include "serra09_locate_kernels.hpp"
#include "serra09_path_kernels.hpp"
#include "chen_align_kernels.hpp"
#include "prep_kernels.hpp"
#include "snf_kernels.hpp"
#include "ef_crossfusion_kernels.hpp"
#include "simple_kernels.hpp"
#include "simple_profile_kernels.hpp"
#include "ef_kernels.hpp"
#include "ef_rowstat2_kernels.hpp"
#include "ef_align_kernels.hpp"
#include "ef_sections_kernels.hpp"
#include "ef_gemm_dma_kernels.hpp"
#include "ef_prep_kernels.hpp"
#include "ftm2d_kernels.hpp"
#include "rank_kernels.hpp"
#include "query_kernels.hpp"
#include "grid.hpp"
#include "query_plan.hpp"
#include "fused_plan.hpp"
#include "snf_batch_kernels.hpp"
#include "serra09_plan.hpp"
#include "ef_plan.hpp"
#include "serra09_sections_kernels.hpp"
#include "device_buffer.hpp"

using acx::PairDesc;
using acx::DeviceBuffer;
using acx::PinnedBuffer;

namespace {

std::string g_create_error;

struct KStat {
    const char *name;
    double ms;
    int64_t launches;
    int64_t cells;
};
enum { KS_OTI = 0, KS_NORMS, KS_BAND, KS_CSM, KS_SEL, KS_QMAX, KS_SIMPLE, KS_EFGEMM, KS_EFSTAT, KS_EFFUSE, KS_EFSW, KS_RANK, KS_TOPK, KS_FTMTILE, KS_QROWS, KS_QTOPK, KS_QRANK, KS_QTOPKL, KS_FTMPAIRS, KS_LOCATE, KS_PATH, KS_SECTIONS, KS_DLOCATE, KS_DPATH, KS_SIMPLEPROF, KS_XFMEANS, KS_XFAFFINITY, KS_XFSNF, KS_XFX, KS_XFSELECT, KS_FUSEDSTAGE, KS_SNFBATCHPREP, KS_SNFBATCHUPDATE, KS_FUSEDROW, KS_EFSECTIONS, KS_EFALIGNLONG, KS_EFALIGN, KS_COUNT };

struct PendingEvent {
    hipEvent_t a, b;
    int stat;
    int64_t cells;
};

// One batch of Serra09 pairs in flight: descriptors, device results and their pinned staging copy.
struct Serra09Slot {
    std::vector<PairDesc> pd, sorted;
    std::vector<int> perm;
    DeviceBuffer<PairDesc> d_pd;
    DeviceBuffer<float> d_out;
    PinnedBuffer<float> h_out;
    PinnedBuffer<int64_t> h_idx;                     // destinations of the batch's scores (grid runs)
    DeviceBuffer<int64_t> d_idx;
    hipEvent_t done = nullptr;
    hipEvent_t cls_ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // a size class's recurrence bitmap is complete
    bool busy = false;
    bool on_q = false;                               // its alignment sweeps run on the context's second stream
    int B = 0, w = 1;
    int64_t k0 = 0;
    // acx_serra09_align: the batch's records instead of scores, and where each pair's strip seam records start in d_seam
    DeviceBuffer<acx_alignment> d_al;
    PinnedBuffer<acx_alignment> h_al;
    std::vector<int64_t> seam_off;
    DeviceBuffer<int64_t> d_seam_off;
    bool al = false;
    // acx_serra09_align_sections: `sec` records per pair in d_al / h_al (0: one, acx_serra09_align's), and how many of them are sections
    int sec = 0;
    DeviceBuffer<int32_t> d_nsec;
    PinnedBuffer<int32_t> h_nsec;
};

}  // namespace

struct acx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t qstream = nullptr;                   // Serra09's alignment sweeps (run_serra09): beside the next band kernels
    hipStream_t qstream2 = nullptr;                  // ... and the second alignment (Dmax) of LateFusionChen beside the first
    hipEvent_t q2_done = nullptr;
    std::string err;
    // pool as uploaded (d_frames0 / d_toff0 / h_off0) and the ACTIVE pool: the upload decimated by the stack stride tau of
    // the last Serra09 call.  d_frames / d_toff hold the decimated copy and are EMPTY at tau == 1, where the active pool is
    // the uploaded one: readers go through active_frames() / active_toff().  Invariant, kept by ensure_tau and free_pool (the
    // only writers of pool_tau): d_frames and d_toff are non-empty exactly when pool_tau > 1, so the accessors may decide by the block.
    DeviceBuffer<float> d_frames0;
    DeviceBuffer<int64_t> d_toff0;
    std::vector<int64_t> h_off0;
    int pool_tau = 0;
    DeviceBuffer<float> d_frames;
    DeviceBuffer<float> d_frot;       // rotated frame pool (band kernel MFMA operands), 36 floats per frame
    DeviceBuffer<_Float16> d_fh;      // the f16 operand pool of the opt-in f16x2 Gram (acx::FH halfs per frame), built on first use
    // the wide class's operand planes (acx::planepool_kernel: 12 planes of acx::FPLANE floats per frame of the ACTIVE pool, each with
    // the pool's slack on both sides), built on first use by ensure_planes and dropped whenever the pool changes
    DeviceBuffer<float> d_planes;
    int64_t plane_floats = 0;         // floats from one plane to the next
    DeviceBuffer<float> d_normtab;    // embedded norms per (track, rotation, frame) for normtab_m / normtab_span
    DeviceBuffer<int64_t> d_noff;
    int normtab_m = 0, normtab_span = -1;
    std::vector<int64_t> h_noff;  // host copy of d_noff (n_tracks + 1 entries; the last one is the table's length)
    DeviceBuffer<int64_t> d_toff;
    DeviceBuffer<float> d_gch;
    std::vector<int64_t> h_off;
    const float *active_frames() const { return d_frames ? d_frames.get() : d_frames0.get(); }
    const int64_t *active_toff() const { return d_toff ? d_toff.get() : d_toff0.get(); }
    int32_t n_tracks = 0, dim = 0;
    // f64 pool (SiMPle)
    DeviceBuffer<double> d_frames64;
    DeviceBuffer<int64_t> d_toff64;
    DeviceBuffer<double> d_prof64;
    DeviceBuffer<double> d_wn64;  // window norms of the f64 pool for subsequence length wn64_L (SiMPle)
    int wn64_L = 0;
    std::vector<int64_t> h_off64;
    int32_t n_tracks64 = 0;
    DeviceBuffer<int32_t> d_pairs;
    DeviceBuffer<double> d_out64;
    // simple_profile_kernel, per chunk of pairs: the records, where each pair's profile starts, the profiles
    // and their indices
    DeviceBuffer<acx::SimpleProfileRec> d_sprec;
    DeviceBuffer<int64_t> d_spoff;
    DeviceBuffer<double> d_spmp;
    DeviceBuffer<int32_t> d_spmpi;
    // EarlyFusion pool
    DeviceBuffer<float> d_ef[3];
    DeviceBuffer<unsigned short> d_efs[3];            // mfcc / ssm / chroma block features as three-term bf16 splits
    int ef_kp[3] = {0, 0, 0};                         // their row length (K rounded up to 32); chroma: bin-major, 0 = no split (f32 kernel)
    DeviceBuffer<float> d_efn[2];
    DeviceBuffer<double> d_efmed;
    DeviceBuffer<int64_t> d_efoff;
    std::vector<int64_t> h_efoff;
    int32_t ef_ntracks = 0;
    int32_t ef_gemm = ACX_EF_GEMM_DEFAULT;            // arithmetic of the three cross-similarity GEMMs
    int32_t ef_fuse = ACX_EF_FUSE_FAST;               // arithmetic of getWCSM's weights and the fused matrix (acx_set_ef_fuse)
    int32_t ef_open = 0;                              // > 0: a pool of that many tracks is being filled (acx_ef_pool_begin .. _end)
    std::vector<uint8_t> ef_filled;                   // per track of the open pool: handed over by acx_ef_pool_tracks yet?
    // FTM2D shingle pool: (ftm_n, ftm_dim) f64, one row per track
    DeviceBuffer<double> d_ftm;
    int32_t ftm_n = 0, ftm_dim = 0;
    int32_t ftm_open = 0;                             // > 0: a pool of that many tracks is being filled (acx_ftm2d_pool_begin .. _end)
    std::vector<uint8_t> ftm_filled;                  // per track of the open pool: handed over by acx_ftm2d_pool_tracks yet?
    acx_ftm2d_params ftm_params = {0.0, 0.0, 0, 0};
    // ranking of score rows (acx_rank_columns / acx_topk_rows): two staging slots of whole rows, pinned + device (grow-only)
    PinnedBuffer<float> rank_h[2];
    DeviceBuffer<float> rank_d[2];
    hipEvent_t rank_ev[2] = {nullptr, nullptr};
    bool rank_attr = false;
    bool query_attr = false;                          // query_topk_kernel's dynamic LDS limit is raised (acx_query_topk)
    bool query_rank_attr = false;                     // query_rank_kernel's (acx_query_ranks)
    bool query_lists_attr = false;                    // query_topk_lists_kernel's (acx_query_topk_lists)
    // multi-GPU inside the library (acx_comm_*): one RCCL communicator rank per context
    ncclComm_t comm = nullptr;
    int comm_rank = 0, comm_world = 0;
    std::vector<DeviceBuffer<char>> dev_bufs;          // acx_dev_alloc'ed buffers still alive (freed with the context)
    int32_t ef_dims[3] = {0, 0, 0};
    DeviceBuffer<acx::EfPair> d_efpd;
    // rectangles of the rectangle GEMM (ef_gemm_rect_bf16x3_kernel): row / column groups, rectangles, pair tables
    DeviceBuffer<acx::EfSegGroup> d_segr, d_segc;
    DeviceBuffer<acx::EfSegRect> d_rects;
    DeviceBuffer<int32_t> d_ptab;
    DeviceBuffer<acx::EfSegWg> d_segw, d_segw2, d_segw3;
    int launch_fail_stat = -1;                         // kernel family (KS_*) of the first failed launch since the last check
    bool ef_rect_attr = false;
    DeviceBuffer<unsigned> d_efctr;                    // tile counters of the persistent rectangle GEMMs (one per launch of a batch)
    int n_cu = 0;
    int ef_split_fmt = 0;                             // what d_efs holds: 0 three bf16 terms, 1 two fp16 terms of x / d_efsc[row]
    DeviceBuffer<float> d_efsc[3];                    // fmt 1: the power-of-two scale of every pool row (ef_rowscale_kernel)
    // scratch (grow-only)
    DeviceBuffer<float> d_scratch, d_thr;
    DeviceBuffer<unsigned> d_efbits;                         // EarlyFusion: the binarised matrices of a batch (ef_rowstat_kernel -> sw_bits_h16_kernel)
    Serra09Slot slot[2];
    DeviceBuffer<float> d_out;
    DeviceBuffer<unsigned long long> d_bits;              // recurrence bitmaps (u64 words)
    DeviceBuffer<acx::LocSeam> d_seam;                    // qmax_locate_kernel's strip seam records (pairs wider than one strip only)
    // qmax_path_kernel, per chunk of boxes: the direction plane (2 bits per box cell), the strip seam records of
    // boxes wider than one strip, the boxes, and the cells and their number as the traceback left them
    DeviceBuffer<unsigned long long> d_dir;
    DeviceBuffer<acx::PathSeam> d_pseam;
    DeviceBuffer<acx::PathBox> d_pbox;
    DeviceBuffer<int32_t> d_pcells, d_pn;
    // ef_align_kernel, per chunk of a batch's pairs: the direction planes (2 bits per cell), the jobs, and the
    // records, cell counts and cells as the kernel left them (one block: one copy per chunk)
    DeviceBuffer<unsigned> d_efdir;
    DeviceBuffer<acx::EfAlignJob> d_efjob;
    DeviceBuffer<int32_t> d_efres;
    int64_t scratch_limit = 0;                            // bytes
    size_t total_mem = 0;
    // the pair grid: last plan (a pure function of lengths and spec; sorting 10^4 tiles per call is what the cache saves)
    std::vector<int64_t> plan_len;
    acx_grid_spec plan_spec = {-1, 0, 0, 0};
    std::vector<acx_grid_tile> plan_tiles;
    DeviceBuffer<int64_t> d_idx;                          // score destinations of a chunk of pairs (grid runs)
    PinnedBuffer<int64_t> h_idx;                          // pinned staging of the same
    DeviceBuffer<char> d_tiles;                           // tile descriptors of a chunk (device-side pair enumeration), bytes
    int nonfinite_policy = ACX_NONFINITE_REJECT;          // what an upload does with NaN / Inf features
    DeviceBuffer<int> d_nf;                               // {first offending track, values zeroed} of the upload scan
    int64_t nf_zeroed = 0;                                // values zeroed by the last upload
    // profiling
    bool prof = false;
    KStat stats[KS_COUNT] = {{"oti_kernel", 0, 0, 0}, {"norms_kernel", 0, 0, 0}, {"band_kernel", 0, 0, 0},
                             {"csm_long_kernel", 0, 0, 0}, {"rowsel_long_kernel", 0, 0, 0}, {"qmax_bits_kernel", 0, 0, 0},
                             {"simple_kernel", 0, 0, 0}, {"ef_gemm_kernel", 0, 0, 0}, {"ef_rowstat_kernel", 0, 0, 0},
                             {"ef_fuse_kernel", 0, 0, 0}, {"sw_kernel", 0, 0, 0}, {"rank_columns_kernel", 0, 0, 0},
                             {"topk_rows_kernel", 0, 0, 0}, {"ftm2d_tile_kernel", 0, 0, 0}, {"query_rows_kernel", 0, 0, 0},
                             {"query_topk_kernel", 0, 0, 0}, {"query_rank_kernel", 0, 0, 0}, {"query_topk_lists_kernel", 0, 0, 0},
                             {"ftm2d_pairs_kernel", 0, 0, 0}, {"qmax_locate_kernel", 0, 0, 0}, {"qmax_path_kernel", 0, 0, 0},
                             {"qmax_sections_kernel", 0, 0, 0},
                             {"dmax_locate_kernel", 0, 0, 0}, {"dmax_path_kernel", 0, 0, 0},
                             {"simple_profile_kernel", 0, 0, 0}, {"xf_means_kernel", 0, 0, 0}, {"xf_affinity_kernels", 0, 0, 0},
                             {"xf_snf_kernels", 0, 0, 0}, {"xf_x_kernel", 0, 0, 0}, {"xf_select_kernel", 0, 0, 0},
                             {"fused_stage_kernel", 0, 0, 0}, {"snf_batch_prepare_kernels", 0, 0, 0}, {"snf_batch_update_kernels", 0, 0, 0},
                             {"fused_row_kernel", 0, 0, 0},
                             {"ef_sections_kernel", 0, 0, 0},
                             {"ef_align_long_kernel", 0, 0, 0},
                             {"ef_align_kernel", 0, 0, 0}};
    std::vector<PendingEvent> pending;
    std::vector<hipEvent_t> event_pool;
    // How many tracks ensure_f16pool's range check saw when it built d_fh (-1: it had no frame to check).  The largest magnitude of
    // a pool that contains those tracks is at least theirs, so the check's lower bound holds for every such pool.
    int32_t fh_base_n = -1;
};

namespace {

int fail(acx_ctx *c, int code, const std::string &msg)
{
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}

#define ACX_HIP(ctx, call)                                                                   \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(ctx, ACX_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

// The one place where a failed (grow-only) allocation becomes ACX_ERR_NOMEM.
template <typename T, bool PINNED>
int ensure(acx_ctx *c, DeviceBuffer<T, PINNED> &buf, size_t need)
{
    const hipError_t e = buf.grow(need);
    if (e != hipSuccess)
        return fail(c, ACX_ERR_NOMEM, std::string(PINNED ? "hipHostMalloc of " : "hipMalloc of ") + std::to_string(need * sizeof(T)) +
                                          " bytes failed: " + hipGetErrorString(e));
    return ACX_OK;
}

// Whole tracks [t0, t1) at a time: a slice takes at least one track and grows while fits(t0, t1) holds and it has fewer than
// max_tracks tracks; body(t0, t1) returns an ACX code, the first that is not ACX_OK ends the loop.
template <typename Fits, typename Body>
int for_track_slices(int n_tracks, int max_tracks, Fits fits, Body body)
{
    for (int t0 = 0; t0 < n_tracks;) {
        int t1 = t0 + 1;
        while (t1 < n_tracks && t1 - t0 < max_tracks && fits(t0, t1 + 1)) ++t1;
        const int rc = body(t0, t1);
        if (rc != ACX_OK) return rc;
        t0 = t1;
    }
    return ACX_OK;
}

hipEvent_t get_event(acx_ctx *c)
{
    if (!c->event_pool.empty()) { hipEvent_t e = c->event_pool.back(); c->event_pool.pop_back(); return e; }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}

struct ProfScope {
    acx_ctx *c; int stat; int64_t cells; hipEvent_t a = nullptr, b = nullptr; hipStream_t st;
    ProfScope(acx_ctx *c_, int stat_, int64_t cells_, hipStream_t st_ = nullptr) : c(c_), stat(stat_), cells(cells_), st(st_ ? st_ : c_->stream)
    {
        if (c->prof) { a = get_event(c); b = get_event(c); (void)hipEventRecord(a, st); }
    }
    ~ProfScope()
    {
        // a launch that failed inside this scope is attributed to the scope's kernel family, not just to the batch (hipPeekAtLastError:
        // the batch's own check still sees and clears it)
        if (c->launch_fail_stat < 0 && hipPeekAtLastError() != hipSuccess) c->launch_fail_stat = stat;
        if (c->prof) { (void)hipEventRecord(b, st); c->pending.push_back({a, b, stat, cells}); }
    }
};

// the batch's launch check: names the kernel family whose scope saw the failure first
#define ACX_LAUNCHES_OK(ctx)                                                                                              \
    do {                                                                                                                  \
        const hipError_t e_ = hipGetLastError();                                                                          \
        if (e_ != hipSuccess) {                                                                                           \
            const int fs_ = (ctx)->launch_fail_stat;                                                                      \
            (ctx)->launch_fail_stat = -1;                                                                                 \
            return fail(ctx, ACX_ERR_HIP, std::string("kernel launch failed (") + (fs_ >= 0 ? (ctx)->stats[fs_].name : "outside the timed scopes") + \
                                              "): " + hipGetErrorString(e_));                                             \
        }                                                                                                                 \
    } while (0)

void drain_profile(acx_ctx *c)
{
    for (auto &p : c->pending) {
        float ms = 0.0f;
        (void)hipEventSynchronize(p.b);
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            c->stats[p.stat].ms += ms;
            c->stats[p.stat].launches += 1;
            c->stats[p.stat].cells += p.cells;
        }
        c->event_pool.push_back(p.a);
        c->event_pool.push_back(p.b);
    }
    c->pending.clear();
}

int round_up(int v, int m) { return (v + m - 1) / m * m; }

// Upload scan for non-finite features (prep_kernels.hpp P0) over `n` values of a packed (rows, dim) device
// array whose first row is row `row_base` of the pool; d_off = the pool's track offsets (device).  Policy
// REJECT: ACX_ERR_INVALID naming the first offending track; ZERO: the values are replaced by 0 in place
// and counted in c->nf_zeroed.  nan_zero_always: NaN is zeroed whatever the policy (MFCCs, as the
// reference does at earlyfusion_traile.py:105).
template <typename T>
int scan_nonfinite(acx_ctx *c, const char *who, const char *what, T *d_x, int64_t n, int dim, int64_t row_base,
                   const int64_t *d_off, int n_tracks, bool nan_zero_always = false, int track_base = 0)
{
    if (n <= 0) return ACX_OK;
    if (const int rc = ensure(c, c->d_nf, 2); rc != ACX_OK) return rc;
    const int init[2] = {0x7fffffff, 0};
    ACX_HIP(c, hipMemcpyAsync(c->d_nf, init, sizeof(init), hipMemcpyHostToDevice, c->stream));
    const bool zero = c->nonfinite_policy == ACX_NONFINITE_ZERO;
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 65536);
    hipLaunchKernelGGL((acx::nonfinite_kernel<T>), dim3(grid), dim3(256), 0, c->stream, d_x, n, dim, row_base, d_off, n_tracks,
                       (zero || nan_zero_always) ? 1 : 0, zero ? 1 : 0, c->d_nf);
    ACX_HIP(c, hipGetLastError());
    int res[2];
    ACX_HIP(c, hipMemcpyAsync(res, c->d_nf, sizeof(res), hipMemcpyDeviceToHost, c->stream));
    ACX_HIP(c, hipStreamSynchronize(c->stream));
    c->nf_zeroed += res[1];
    if (res[0] != 0x7fffffff)
        return fail(c, ACX_ERR_INVALID, std::string(who) + ": track " + std::to_string(track_base + res[0]) + " holds a non-finite value (NaN / Inf) in its " +
                    what + "; clean the features or select acx_set_nonfinite_policy(ctx, ACX_NONFINITE_ZERO)");
    return ACX_OK;
}

int check_params(acx_ctx *c, const acx_serra09_params &p)
{
    if (p.m < 1 || p.m > acx::MAX_M_LONG) return fail(c, ACX_ERR_UNSUPPORTED, "serra09: m must be in 1..33 on the device");
    if (p.tau < 1) return fail(c, ACX_ERR_INVALID, "serra09: tau must be >= 1");
    if (!(p.kappa >= 0.0f && p.kappa <= 1.0f)) return fail(c, ACX_ERR_INVALID, "serra09: kappa must be in [0, 1]");
    if (p.dp_start != 2 && p.dp_start != 3) return fail(c, ACX_ERR_INVALID, "serra09: dp_start must be 2 or 3");
    if (p.pct_mode < 0 || p.pct_mode > 3) return fail(c, ACX_ERR_INVALID, "serra09: pct_mode must be 0..3");
    if (p.oti_target != 0 && p.oti_target != 1) return fail(c, ACX_ERR_INVALID, "serra09: oti_target must be 0 or 1");
    if (!(p.gamma_o >= 0.0f) || !(p.gamma_e >= 0.0f)) return fail(c, ACX_ERR_INVALID, "serra09: gammas must be >= 0");
    if (p.arith != ACX_ARITH_EXACT && p.arith != ACX_ARITH_F16X2) return fail(c, ACX_ERR_INVALID, "serra09: arith must be ACX_ARITH_EXACT or ACX_ARITH_F16X2");
    if (p.arith == ACX_ARITH_F16X2 && p.m != 9) return fail(c, ACX_ERR_UNSUPPORTED, "serra09: the f16x2 Gram exists for the default stack size m = 9 only");
    return ACX_OK;
}

// The band kernel's edge tiles read their operands and norms WITHOUT clamping the frame index (the cells
// they feed are masked anyway): up to 7 frames before a track and 71 behind it.  Inside the pool that is
// a neighbouring track; the two ends of the rotated pool and of the norm table carry this much zeroed slack.
constexpr int64_t POOL_SLACK = 96;      // frames (rotated pool) / floats (norm table) on either side

// band_kernel is launched from its own translation unit (acx_band.hip)
// (hpd: the host's copy of the same B descriptors, for the plan's per-launch decisions)
bool launch_band(acx_ctx *c, int m, const PairDesc *dpd, const std::vector<PairDesc> &hpd, int b0, int B, int maxRows, int cls,
                 const acx_serra09_params &p, int role, int write_d2, int want_eps)
{
    const float *operands = p.arith == ACX_ARITH_F16X2 ? reinterpret_cast<const float *>(c->d_fh + POOL_SLACK * acx::FH) : c->d_frot + POOL_SLACK * acx::FROT;
    acx::BandLaunch L{c->stream, operands, c->active_toff(), c->d_normtab + POOL_SLACK, c->d_noff, c->d_scratch, c->d_thr,
                      c->d_bits, p.kappa, p.pct_mode, p.inclusive, p.oti_target,
                      c->d_planes ? c->d_planes + POOL_SLACK * acx::FPLANE : nullptr, c->plane_floats, 0};
    const int family = acx::serra09_band_family(cls, m, p.arith);
    bool ok = true;
    for (const acx::Serra09Run &r : acx::serra09_fast_tail_runs(p, family, role, write_d2 != 0, want_eps != 0, c->d_bits != nullptr, hpd, b0, b0 + B)) {
        L.fast_tail = r.fast ? 1 : 0;
        ok = ok && acx::launch_band_kernel(L, m, dpd + (r.begin - b0), r.end - r.begin, maxRows, family, role, write_d2, want_eps, p.arith);
    }
    return ok;
}

template <int M>
void launch_normtab(acx_ctx *c, int maxM, int span, int first, int count)       // tracks [first, first + count) of the active pool
{
    hipLaunchKernelGGL((acx::normtab_kernel<M>), dim3(count, (maxM + 255) / 256, acx::NBIN), dim3(256), 0, c->stream,
                       c->active_frames(), c->active_toff() + first, c->d_noff + first, c->d_normtab + POOL_SLACK, span);
}

#ifdef ACX_FAST_BUILD   /* development builds: only the default stack size */
#ifndef ACX_FAST_BUILD_M
#define ACX_FAST_BUILD_M 9
#endif
#define ACX_M_SWITCH(m_, CALL) switch (m_) { case ACX_FAST_BUILD_M: CALL(ACX_FAST_BUILD_M); break; default: handled = false; }
#else
#define ACX_M_SWITCH(m_, CALL)                                                                      \
    switch (m_) {                                                                                   \
        case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break;     \
        case 5: CALL(5); break; case 6: CALL(6); break; case 7: CALL(7); break; case 8: CALL(8); break;     \
        case 9: CALL(9); break; case 10: CALL(10); break; case 11: CALL(11); break; case 12: CALL(12); break; \
        case 13: CALL(13); break; case 14: CALL(14); break; case 15: CALL(15); break; case 16: CALL(16); break; \
        default: handled = false;                                                                   \
    }
#endif

// The active pool is the uploaded one decimated by the stack stride: the stack at base frame e tau
// holds frames (e + k) tau, so with X'[t] = X[t tau] it is the tau = 1 stack of X' (same frames,
// same order, same count: ceil(T / tau) - m = ceil((T - m tau) / tau)).  The OTI's global chroma
// stays the one of the complete track.  Rebuilt when tau changes; at tau = 1 the upload is the active pool.
int ensure_tau(acx_ctx *c, int tau)
{
    if (c->pool_tau == tau) return ACX_OK;
    c->normtab_m = 0; c->normtab_span = -1;      // the keys first: a reset that fails below leaves no key on an emptied block
    c->pool_tau = 0;
    c->fh_base_n = -1;
    ACX_HIP(c, c->d_frames.reset());
    ACX_HIP(c, c->d_toff.reset());
    ACX_HIP(c, c->d_frot.reset());
    ACX_HIP(c, c->d_fh.reset());
    ACX_HIP(c, c->d_planes.reset());
    ACX_HIP(c, c->d_normtab.reset());
    ACX_HIP(c, c->d_noff.reset());
    const int n = c->n_tracks;
    DeviceBuffer<float> frames, frot;            // built here and moved into the context when complete: a failure leaves no half-built pool
    DeviceBuffer<int64_t> toff;
    if (tau == 1) {
        c->h_off = c->h_off0;
    } else {
        c->h_off.assign((size_t)n + 1, 0);
        int maxT = 1;
        for (int t = 0; t < n; ++t) {
            const int64_t T = c->h_off0[t + 1] - c->h_off0[t];
            const int64_t Td = (T + tau - 1) / tau;
            c->h_off[t + 1] = c->h_off[t] + Td;
            maxT = std::max<int>(maxT, (int)Td);
        }
        const int64_t total = c->h_off[n];
        ACX_HIP(c, frames.grow((size_t)std::max<int64_t>(1, total) * acx::NBIN));
        ACX_HIP(c, toff.grow((size_t)n + 1));
        ACX_HIP(c, hipMemcpy(toff, c->h_off.data(), sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice));
        if (total > 0) {
            hipLaunchKernelGGL(acx::decimate_kernel, dim3(n, (maxT * acx::NBIN + 255) / 256), dim3(256), 0, c->stream,
                               c->d_frames0.get(), c->d_toff0.get(), toff.get(), frames.get(), tau);
            ACX_HIP(c, hipGetLastError());
        }
    }
    const int64_t total = c->h_off[n];
    const float *active = tau == 1 ? c->d_frames0.get() : frames.get();
    // rotated copy of the active pool: the band kernel loads its MFMA operands from it (12 bytes per
    // lane per 16-frame tile, already in the rotated chain order) -- 144 B per frame
    ACX_HIP(c, frot.grow((size_t)(std::max<int64_t>(1, total) + 2 * POOL_SLACK) * acx::FROT));
    ACX_HIP(c, hipMemsetAsync(frot, 0, sizeof(float) * POOL_SLACK * acx::FROT, c->stream));
    ACX_HIP(c, hipMemsetAsync(frot + (POOL_SLACK + total) * acx::FROT, 0, sizeof(float) * POOL_SLACK * acx::FROT, c->stream));
    if (total > 0) {
        const int64_t nout = total * acx::FROT;
        hipLaunchKernelGGL(acx::rotpool_kernel, dim3((unsigned)std::min<int64_t>((nout + 255) / 256, 1 << 22)), dim3(256), 0, c->stream,
                           active, frot + POOL_SLACK * acx::FROT, total);
        ACX_HIP(c, hipGetLastError());
    }
    ACX_HIP(c, hipStreamSynchronize(c->stream));
    c->d_frames = std::move(frames);             // (both empty at tau == 1)
    c->d_toff = std::move(toff);
    c->d_frot = std::move(frot);
    c->pool_tau = tau;
    return ACX_OK;
}

// The f16 operand pool of the opt-in f16x2 Gram (192 B per frame of the ACTIVE pool): built on first use, dropped with the pool.
// largest |x| of a float array as a bit pattern (|x| patterns order like the values)
static __global__ void absmax_kernel(const float *__restrict__ v, int64_t n, unsigned *__restrict__ out)
{
    unsigned m = 0u;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        m = max(m, __float_as_uint(v[i]) & 0x7fffffffu);
    for (int o = 32; o >= 1; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

constexpr float F16X2_MIN_MAX = 0.5f, F16X2_MAX_MAX = 32768.0f;     // the range of a pool's largest magnitude, here and in s09_append_derived's copy of the check

int ensure_f16pool(acx_ctx *c)
{
    if (c->d_fh) return ACX_OK;
    const int64_t total = c->h_off[c->n_tracks];
    // The two-term fp16 split x = h1 + h2 carries 22 bits only while h1 is finite and h2 keeps its bits: features above 65504 would
    // become inf (NaN distances), and h2 = fp16(x - h1) is rounded to fp16's subnormal step of 2^-24 -- an ABSOLUTE error, so every
    // halving of the features doubles the error of 2 xy relative to them, while the embedded norms, made from the exact f32
    // values, no longer match the Gram.  At a largest value of 1 that step is the smaller part of the error; from 2^-2 down it
    // dominates (2 xy of frame-max-normalised chroma: 1.95e-6 at 1, 2.6e-6 at 2^-1, 5.3e-6 at 2^-2, 2.8e-4 at 2^-8, which was the
    // limit once; tests/test_serra09_f64_ref.py derives it, tests/test_gpu_serra09_f16x2.py holds d2 to 3e-5 over the whole range).
    // HPCP / CREMA frames are normalised to a maximum of 1; a pool whose largest value lies outside [2^-1, 2^15] is refused
    // (rescale it by a power of two, or use ACX_ARITH_EXACT).
    unsigned h_m = 0u;
    if (total > 0) {
        DeviceBuffer<unsigned> d_m;
        ACX_HIP(c, d_m.grow(1));
        ACX_HIP(c, hipMemsetAsync(d_m, 0, sizeof(unsigned), c->stream));
        hipLaunchKernelGGL(absmax_kernel, dim3((unsigned)std::min<int64_t>((total * acx::NBIN + 255) / 256, 4096)), dim3(256), 0, c->stream,
                           c->active_frames(), total * acx::NBIN, d_m.get());
        ACX_HIP(c, hipMemcpyAsync(&h_m, d_m, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
        ACX_HIP(c, hipStreamSynchronize(c->stream));
        float mx;
        memcpy(&mx, &h_m, sizeof(mx));
        if (!(mx >= F16X2_MIN_MAX && mx <= F16X2_MAX_MAX))
            return fail(c, ACX_ERR_UNSUPPORTED, "serra09: arith = f16x2 needs features whose largest magnitude lies in [2^-1, 2^15] (this pool: " +
                                                    std::to_string(mx) + "; below 2^-1 the second fp16 term loses its bits to the subnormal "
                                                    "step and the distances their accuracy): rescale the pool by a power of two or use the exact arithmetic");
    }
    const size_t halfs = (size_t)(std::max<int64_t>(1, total) + 2 * POOL_SLACK) * acx::FH;
    DeviceBuffer<_Float16> fh;                         // the context's once it is complete
    const hipError_t e = fh.grow(halfs);
    if (e != hipSuccess) return fail(c, ACX_ERR_NOMEM, std::string("serra09: the f16 operand pool does not fit the device: ") + hipGetErrorString(e));
    ACX_HIP(c, hipMemsetAsync(fh, 0, sizeof(_Float16) * halfs, c->stream));
    if (total > 0) {
        hipLaunchKernelGGL(acx::rotpool_f16_kernel, dim3((unsigned)std::min<int64_t>((total * 12 + 255) / 256, 1 << 22)), dim3(256), 0, c->stream,
                           c->active_frames(), fh + POOL_SLACK * acx::FH, total);
        ACX_HIP(c, hipGetLastError());
    }
    ACX_HIP(c, hipStreamSynchronize(c->stream));
    c->d_fh = std::move(fh);
    c->fh_base_n = total > 0 ? c->n_tracks : -1;
    return ACX_OK;
}

// The operand planes of the wide class (exact arithmetic): 12 x 48 B per frame of the ACTIVE pool on top of the rotated pool's 144 B,
// so they are built on the first batch that launches that class, from the rotated pool, and only while ACX_PLANES is not 0.  A plane
// carries the pool's slack on both sides (zeroed: what the edge tiles of the first and the last track read).  The distance between
// planes depends on the pool's length, so every change of the pool (ensure_tau, append, truncate, a new upload) drops them and the
// next wide batch builds them again.
int ensure_planes(acx_ctx *c)
{
    if (c->d_planes || !acx::serra09_switches().planes) return ACX_OK;
    const int64_t total = c->h_off[c->n_tracks];
    const int64_t plane_floats = (std::max<int64_t>(1, total) + 2 * POOL_SLACK) * acx::FPLANE;
    DeviceBuffer<float> planes;                        // the context's once it is complete
    const hipError_t e = planes.grow((size_t)plane_floats * acx::NBIN);
    if (e != hipSuccess)
        return fail(c, ACX_ERR_NOMEM, std::string("serra09: the wide class's operand planes (576 bytes per pooled frame) do not fit the device: ") +
                                          hipGetErrorString(e) + "; ACX_PLANES=0 runs that class from the rotated pool");
    ACX_HIP(c, hipMemsetAsync(planes, 0, sizeof(float) * (size_t)plane_floats * acx::NBIN, c->stream));
    if (total > 0) {
        const int64_t nout = total * acx::FPLANE * acx::NBIN;
        hipLaunchKernelGGL(acx::planepool_kernel, dim3((unsigned)std::min<int64_t>((nout + 255) / 256, 1 << 22)), dim3(256), 0, c->stream,
                           c->d_frot + POOL_SLACK * acx::FROT, planes + POOL_SLACK * acx::FPLANE, total, plane_floats);
        ACX_HIP(c, hipGetLastError());
    }
    ACX_HIP(c, hipStreamSynchronize(c->stream));
    c->d_planes = std::move(planes);
    c->plane_floats = plane_floats;
    return ACX_OK;
}

// The table of embedded norms depends on the pool and on (m, embedded length): built on first use.
int ensure_normtab(acx_ctx *c, const acx_serra09_params &p)
{
    const int span = p.embed_full ? (p.m - 1) : p.m;           // (active pool: tau == 1)
    if (c->d_normtab && c->normtab_m == p.m && c->normtab_span == span) return ACX_OK;
    ACX_HIP(c, c->d_normtab.reset());
    ACX_HIP(c, c->d_noff.reset());
    c->normtab_m = 0; c->normtab_span = -1;            // (a failure below must not leave the old key on a new, unfinished table)
    std::vector<int64_t> &noff = c->h_noff;
    noff.assign((size_t)c->n_tracks + 1, 0);
    int64_t tot = 0;
    int maxM = 1;
    for (int t = 0; t < c->n_tracks; ++t) {
        noff[t] = tot;
        const int Me = std::max<int>(0, (int)(c->h_off[t + 1] - c->h_off[t]) - span);
        maxM = std::max(maxM, Me);
        tot += (int64_t)acx::NBIN * (Me + acx::NGUARD);      // + the +inf guard entries behind every rotation's row
    }
    noff[c->n_tracks] = tot;
    ACX_HIP(c, c->d_normtab.grow((size_t)(std::max<int64_t>(1, tot) + 2 * POOL_SLACK)));
    // +inf everywhere first: the guard entries and the slack are what the band kernel reads for columns outside a matrix
    ACX_HIP(c, hipMemsetD32Async((hipDeviceptr_t)c->d_normtab, 0x7f800000, (size_t)(std::max<int64_t>(1, tot) + 2 * POOL_SLACK), c->stream));
    ACX_HIP(c, c->d_noff.grow(noff.size()));
    ACX_HIP(c, hipMemcpy(c->d_noff, noff.data(), sizeof(int64_t) * noff.size(), hipMemcpyHostToDevice));
    bool handled = true;
    {
        ProfScope ps(c, KS_NORMS, 0);
#define ACX_CALL(M_) launch_normtab<M_>(c, maxM, span, 0, c->n_tracks)
        ACX_M_SWITCH(p.m, ACX_CALL)
#undef ACX_CALL
    }
    if (!handled) return fail(c, ACX_ERR_UNSUPPORTED, "serra09: this build of libacx has no band kernel for the requested m");
    ACX_HIP(c, hipGetLastError());
    c->normtab_m = p.m;
    c->normtab_span = span;
    return ACX_OK;
}

struct DebugOut {
    float *d2, *epsq, *epsr, *thrq, *thrr;
    int32_t *oti;
    int32_t *dims;
};

int64_t scratch_limit_bytes(const acx_ctx *c)
{
    if (c->scratch_limit > 0) return c->scratch_limit;
    const char *env = getenv("ACX_SCRATCH_GB");
    if (env && atof(env) > 0) return (int64_t)(atof(env) * (double)(1ull << 30));
    // (the wide class's operand planes are the one derived pool larger than the features themselves -- 17 GB for 15 000 tracks of
    // 2000 frames: the default share is taken of what they leave)
    return (int64_t)(0.40 * (double)(c->total_mem - (int64_t)(c->d_planes.capacity() * sizeof(float))));
}

// Results of one batch come back through a pinned staging slot; two slots, so that the host packs
// batch b + 1 (descriptors, size classes) while the device works on batch b.
int collect_slot(acx_ctx *c, Serra09Slot &s, float *out, acx_alignment *al = nullptr, int32_t *nsec = nullptr)
{
    if (!s.busy) return ACX_OK;
    ACX_HIP(c, hipEventSynchronize(s.done));
    for (int k2 = 0; s.al && !s.sec && al && k2 < s.B; ++k2) al[s.k0 + s.perm[k2]] = s.h_al[(size_t)k2];
    for (int k2 = 0; s.al && s.sec && al && nsec && k2 < s.B; ++k2) {      // (the sections of a pair stay together)
        const size_t k = (size_t)(s.k0 + s.perm[k2]);
        for (int e = 0; e < s.sec; ++e) al[k * s.sec + e] = s.h_al[(size_t)k2 * s.sec + e];
        nsec[k] = s.h_nsec[(size_t)k2];
    }
    for (int k2 = 0; !s.al && out && k2 < s.B; ++k2)
        for (int e = 0; e < s.w; ++e) out[(size_t)s.w * (s.k0 + s.perm[k2]) + e] = s.h_out[(size_t)s.w * k2 + e];
    s.busy = false;
    drain_profile(c);
    return ACX_OK;
}

// Scores go to a DEVICE buffer instead of the host: pair k's `w` values to base[idx[k] .. + w)
struct DevDst {
    float *base;
    const int64_t *idx;
};

static __global__ void scatter_scores_kernel(const float *__restrict__ src, const int64_t *__restrict__ idx,
                                             float *__restrict__ dst, int B, int w)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= B) return;
    for (int e = 0; e < w; ++e) dst[idx[k] + e] = src[(size_t)k * w + e];
}

static __global__ void scatter_f64_kernel(const double *__restrict__ src, const int64_t *__restrict__ idx, float *__restrict__ dst, int n)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) dst[idx[k]] = (float)src[k];          // the f32 store of Ds['main'][i, j] = sim (simple_silva.py:125-126)
}

// The pairs of a chunk of grid tiles, enumerated ON THE DEVICE (no host pair list, no sort, no upload):
// tile t's pairs land at [pair_base, pair_base + P) in COLUMN-major order -- second track slowest, which is
// the order simple_kernel wants its pairs in (neighbouring waves walk the same track B).  A diagonal tile of
// a symmetric grid holds i < j only (column b has b pairs), of an ordered grid i != j (n - 1 per column).
struct TileDev {
    int32_t row0, col0, rows, cols;
    int32_t diagonal, pad;
    int64_t offset;        // float offset of the tile in the rank's score buffer
    int64_t pair_base;     // first pair of the tile in the chunk
};

static __host__ __device__ inline int64_t tile_pair_count(int rows, int cols, int diagonal, int symmetric)
{
    if (!diagonal) return (int64_t)rows * cols;
    return symmetric ? (int64_t)rows * (rows - 1) / 2 : (int64_t)rows * (rows - 1);
}

static __global__ void grid_pairs_kernel(const TileDev *__restrict__ tiles, int symmetric, int w, int32_t *__restrict__ pairs,
                                         int64_t *__restrict__ idx)
{
    const TileDev t = tiles[blockIdx.y];
    const int64_t P = tile_pair_count(t.rows, t.cols, t.diagonal, symmetric);
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < P; k += (int64_t)gridDim.x * blockDim.x) {
        int a, b;
        if (!t.diagonal) {
            b = (int)(k / t.rows); a = (int)(k - (int64_t)b * t.rows);
        } else if (symmetric) {
            b = (int)((1.0 + __builtin_sqrt(1.0 + 8.0 * (double)k)) * 0.5);
            while ((int64_t)b * (b - 1) / 2 > k) --b;
            while ((int64_t)(b + 1) * b / 2 <= k) ++b;
            a = (int)(k - (int64_t)b * (b - 1) / 2);
        } else {
            b = (int)(k / (t.rows - 1)); a = (int)(k - (int64_t)b * (t.rows - 1));
            a += (a >= b) ? 1 : 0;
        }
        pairs[2 * (t.pair_base + k)] = t.row0 + a;
        pairs[2 * (t.pair_base + k) + 1] = t.col0 + b;
        idx[t.pair_base + k] = t.offset + ((int64_t)a * t.cols + b) * w;
    }
}

// A call that fails half way must not leave work in flight behind its error code: every stream the chain uses is drained
// (the next call's row pass writes the bitmap arena the old sweeps may still be reading) and no slot stays marked busy
// with results nobody will collect.  The reference fails the whole chunk of pairs (algorithm_template.py:174-177); so does this.
void quiesce(acx_ctx *c)
{
    (void)hipStreamSynchronize(c->stream);
    if (c->qstream) (void)hipStreamSynchronize(c->qstream);
    if (c->qstream2) (void)hipStreamSynchronize(c->qstream2);
    for (Serra09Slot &sl : c->slot) sl.busy = false;
    (void)hipGetLastError();
    drain_profile(c);
}

// The guard of every entry point that queues work: body() returns an ACX code, and any code but ACX_OK is returned with the streams
// idle -- no queued copy still reads a host buffer of the call that is about to go out of scope, or still writes the caller's.
template <typename Body>
int guarded(acx_ctx *c, Body body)
{
    const int rc = body();
    if (rc != ACX_OK) quiesce(c);                // (c->err keeps the first failure's text)
    return rc;
}

// The tracebacks on the device wrote the cells end first: the n cells of `src`, from the start to the end, into dst.
void reverse_cells(const int32_t *src, int n, int32_t *dst)
{
    for (int t = 0; t < n; ++t) { dst[2 * (size_t)t] = src[2 * (n - 1 - t)]; dst[2 * (size_t)t + 1] = src[2 * (n - 1 - t) + 1]; }
}

// The WHOLE pair list is checked before the first launch: indices, tracks shorter than the stack, pairs that cannot fit the
// scratch limit on their own.  (The batch loop used to find these when it reached them -- with earlier batches in flight.)
int validate_serra09_pairs(acx_ctx *c, const acx::Serra09Lengths &len, const int32_t *pairs, int64_t K, const acx_serra09_params &p, bool dbg,
                           int64_t limit_floats)
{
    int64_t k = 0;
    switch (acx::serra09_check_pairs(len, pairs, K, p, dbg, limit_floats, &k)) {
    case ACX_ERR_INVALID: return fail(c, ACX_ERR_INVALID, "serra09: track index out of range in pair " + std::to_string(k));
    case ACX_ERR_SHORT: return fail(c, ACX_ERR_SHORT, "serra09: track shorter than the delay-embedding stack (pair " + std::to_string(k) + ")");
    case ACX_ERR_NOMEM: return fail(c, ACX_ERR_NOMEM, "serra09: pair " + std::to_string(k) + " does not fit the scratch limit");
    }
    return ACX_OK;
}

// One alignment sweep (Qmax, or Dmax) over the recurrence bitmaps of B pairs, one wave per pair: pair k's score goes to dst[k w].
// cols: bitmap columns a lane owns -- 8 / 16 / 32 for rows of up to 505 / 1017 / 2041 cells, 0: the long kernel (any length; its strip
// records live in `scratch`).  pack: 4 / 2 pairs share a wave (rows of <= 249 / 505 cells, the default penalties only); 1: one wave
// per pair.  Both come from the size class's row of serra09_plan.hpp (serra09_sweep).  The default penalties (0.5 / 0.5) take the
// packed 16-bit integer DP in half-units, two cells per instruction.
void launch_qmax_sweep(hipStream_t st, const PairDesc *pd, int B, const unsigned long long *bits, float *scratch, float *dst, int w,
                       float gamma_o, float gamma_e, int dp_start, bool dmax, int cols, int pack)
{
#define ACX_QB3(E_, D_, C_) hipLaunchKernelGGL((acx::qmax_bits_kernel<E_, D_, C_>), dim3(B), dim3(64), 0, st, pd, bits, dst, w, gamma_o, gamma_e, dp_start)
#define ACX_QBL(E_, D_) hipLaunchKernelGGL((acx::qmax_bits_long_kernel<E_, D_>), dim3(B), dim3(64), 0, st, pd, bits, scratch, dst, w, gamma_o, gamma_e, dp_start)
#define ACX_QB(E_, D_) do { if (cols == 8) ACX_QB3(E_, D_, 8); else if (cols == 16) ACX_QB3(E_, D_, 16); else if (cols == 32) ACX_QB3(E_, D_, 32); \
                            else ACX_QBL(E_, D_); } while (0)
#define ACX_QH(C_, D_) hipLaunchKernelGGL((acx::qmax_bits_h16_kernel<C_, D_>), dim3(B), dim3(64), 0, st, pd, bits, dst, w, dp_start)
#define ACX_QM(G_, D_) hipLaunchKernelGGL((acx::qmax_bits_h16_multi_kernel<G_, D_>), dim3((B + 64 / G_ - 1) / (64 / G_)), dim3(64), 0, st, \
                                          pd, B, bits, dst, w, dp_start)
    const bool eqg = gamma_o == gamma_e;
    if (eqg && gamma_o == 0.5f && cols != 0) {
        if (pack == 4) { if (dmax) ACX_QM(16, true); else ACX_QM(16, false); }
        else if (pack == 2) { if (dmax) ACX_QM(32, true); else ACX_QM(32, false); }
        else if (dmax) { if (cols == 8) ACX_QH(8, true); else if (cols == 16) ACX_QH(16, true); else ACX_QH(32, true); }
        else { if (cols == 8) ACX_QH(8, false); else if (cols == 16) ACX_QH(16, false); else ACX_QH(32, false); }
    }
    else if (eqg) { if (dmax) ACX_QB(true, true); else ACX_QB(true, false); }
    else { if (dmax) ACX_QB(false, true); else ACX_QB(false, false); }
#undef ACX_QM
#undef ACX_QH
#undef ACX_QB
#undef ACX_QBL
#undef ACX_QB3
}

// The locating sweep (serra09_locate_kernels.hpp) over the recurrence bitmaps of B pairs, one wave per pair of any shape: pair k's
// record goes to dst[k]; seam_off[k] = first of its strip seam records in `seam` (read for pairs wider than one strip only).
void launch_qmax_locate(hipStream_t st, const PairDesc *pd, int B, const unsigned long long *bits, acx::LocSeam *seam, const int64_t *seam_off,
                        acx_alignment *dst, float gamma_o, float gamma_e, int dp_start)
{
    if (gamma_o == gamma_e)
        hipLaunchKernelGGL((acx::qmax_locate_kernel<true>), dim3(B), dim3(64), 0, st, pd, bits, seam, seam_off, dst, gamma_o, gamma_e, dp_start);
    else
        hipLaunchKernelGGL((acx::qmax_locate_kernel<false>), dim3(B), dim3(64), 0, st, pd, bits, seam, seam_off, dst, gamma_o, gamma_e, dp_start);
}

// What acx_serra09_align_sections adds to an alignment run (run_serra09_impl's `sec`).
struct SectionRun {
    acx_section_opts o;
    int32_t *n;            // where the pairs' section counts go (K of them, in the order of the list)
};

// Every section of B pairs (serra09_sections_kernels.hpp), one wave per pair and one launch: pair k's o.max_sections records go to
// dst[k * o.max_sections ..], their number to n_dst[k]; bitmaps and seam records as for launch_qmax_locate.
void launch_qmax_sections(hipStream_t st, const PairDesc *pd, int B, const unsigned long long *bits, acx::LocSeam *seam, const int64_t *seam_off,
                          acx_alignment *dst, int32_t *n_dst, float gamma_o, float gamma_e, int dp_start, const acx_section_opts &o)
{
    if (gamma_o == gamma_e)
        hipLaunchKernelGGL((acx::qmax_sections_kernel<true>), dim3(B), dim3(64), 0, st, pd, bits, seam, seam_off, dst, n_dst, gamma_o, gamma_e,
                           dp_start, o.max_sections, o.pad, o.min_score, o.min_ratio);
    else
        hipLaunchKernelGGL((acx::qmax_sections_kernel<false>), dim3(B), dim3(64), 0, st, pd, bits, seam, seam_off, dst, n_dst, gamma_o, gamma_e,
                           dp_start, o.max_sections, o.pad, o.min_score, o.min_ratio);
}

// The same for the Dmax alignment (chen_align_kernels.hpp): same records, same seam buffer.
void launch_dmax_locate(hipStream_t st, const PairDesc *pd, int B, const unsigned long long *bits, acx::LocSeam *seam, const int64_t *seam_off,
                        acx_alignment *dst, float gamma_o, float gamma_e, int dp_start)
{
    if (gamma_o == gamma_e)
        hipLaunchKernelGGL((acx::dmax_locate_kernel<true>), dim3(B), dim3(64), 0, st, pd, bits, seam, seam_off, dst, gamma_o, gamma_e, dp_start);
    else
        hipLaunchKernelGGL((acx::dmax_locate_kernel<false>), dim3(B), dim3(64), 0, st, pd, bits, seam, seam_off, dst, gamma_o, gamma_e, dp_start);
}

// The path pass (serra09_path_kernels.hpp) behind a locating sweep, while c->d_bits still holds the bitmaps of the B pairs whose
// descriptors are `dpd` on the device: recs[k2] is pair k2's record ON THE HOST (the caller has waited for it), and pair k2's cells
// go to dst(k2) as (q, r) from start to end; a pair without a match gets none.  The boxes run in CHUNKS: as many consecutive boxes as
// fit path_budget_bytes (direction planes + seam records) and one launch's grid; a single box beyond it is ACX_ERR_NOMEM (`name(k2)`
// says which pair).  Runs on the main stream and returns with it idle.  `dmax`: the records are a Dmax locating sweep's and the pass is
// dmax_path_kernel (same boxes, planes, records and budget).  `per` (acx_serra09_align_sections): every pair has `per` records, record
// k2 being section k2 % per of pair k2 / per -- its box names that pair's descriptor -- and dst / name take the record's index.
int64_t path_budget_bytes(const acx_ctx *c) { return scratch_limit_bytes(c) / 2; }

template <typename Dst, typename Name>
int run_qmax_paths(acx_ctx *c, const PairDesc *dpd, const acx_alignment *recs, int B, float gamma_o, float gamma_e, Dst dst, Name name,
                   bool dmax = false, int per = 1)
{
    const std::string who = dmax ? "dmax_path: " : "qmax_path: ";
    const int64_t budget = path_budget_bytes(c);
    std::vector<acx::PathBox> boxes;
    std::vector<int> owner;
    std::vector<int32_t> h_n, h_cells;
    int k2 = 0;
    B *= per;
    while (k2 < B) {
        boxes.clear(); owner.clear();
        int64_t words = 0, seams = 0, ncell = 0, bytes = 0, area = 0;
        for (; k2 < B && boxes.size() < 65535; ++k2) {
            const acx_alignment &a = recs[k2];
            dst(k2).clear();
            if (!(a.score > 0.0f) || a.q0 < 0) continue;
            const int rows = a.q1 - a.q0 + 1, width = a.r1 - a.r0 + 1;
            if (rows < 1 || width < 1 || a.r0 < 0) return fail(c, ACX_ERR_STATE, who + "pair " + name(k2) + " has a malformed alignment record");
            const int64_t need = acx::path_box_bytes(rows, width);
            if (need > budget)
                return fail(c, ACX_ERR_NOMEM, who + "the " + std::to_string(rows) + " x " + std::to_string(width) + " box of pair " + name(k2) +
                                                  " takes " + std::to_string(need) + " bytes, beyond the path budget of " + std::to_string(budget) +
                                                  " (half the scratch limit)");
            if (bytes + need > budget) break;
            acx::PathBox bx;
            bx.pair = k2 / per; bx.q0 = a.q0; bx.r0 = a.r0; bx.q1 = a.q1; bx.r1 = a.r1;
            bx.max_cells = std::min(rows, width);
            bx.dir_off = words; bx.seam_off = seams; bx.cell_off = ncell;
            words += (int64_t)rows * acx::path_words(width);
            if (acx::path_strips(width) > 1) seams += 2 * (int64_t)rows;
            ncell += bx.max_cells;
            bytes += need;
            area += (int64_t)rows * width;
            boxes.push_back(bx); owner.push_back(k2);
        }
        const int nb = (int)boxes.size();
        if (nb == 0) continue;
        int rc;
        if ((rc = ensure(c, c->d_dir, (size_t)words)) != ACX_OK) return rc;
        if ((rc = ensure(c, c->d_pseam, (size_t)std::max<int64_t>(seams, 1))) != ACX_OK) return rc;
        if ((rc = ensure(c, c->d_pbox, (size_t)nb)) != ACX_OK) return rc;
        if ((rc = ensure(c, c->d_pcells, (size_t)(2 * ncell))) != ACX_OK) return rc;
        if ((rc = ensure(c, c->d_pn, (size_t)nb)) != ACX_OK) return rc;
        ACX_HIP(c, hipMemcpyAsync(c->d_pbox, boxes.data(), sizeof(acx::PathBox) * nb, hipMemcpyHostToDevice, c->stream));
        {
            ProfScope ps(c, dmax ? KS_DPATH : KS_PATH, area);
            if (dmax && gamma_o == gamma_e)
                hipLaunchKernelGGL((acx::dmax_path_kernel<true>), dim3(nb), dim3(64), 0, c->stream, dpd, c->d_pbox, c->d_bits, c->d_dir, c->d_pseam,
                                   c->d_pcells, c->d_pn, gamma_o, gamma_e);
            else if (dmax)
                hipLaunchKernelGGL((acx::dmax_path_kernel<false>), dim3(nb), dim3(64), 0, c->stream, dpd, c->d_pbox, c->d_bits, c->d_dir, c->d_pseam,
                                   c->d_pcells, c->d_pn, gamma_o, gamma_e);
            else if (gamma_o == gamma_e)
                hipLaunchKernelGGL((acx::qmax_path_kernel<true>), dim3(nb), dim3(64), 0, c->stream, dpd, c->d_pbox, c->d_bits, c->d_dir, c->d_pseam,
                                   c->d_pcells, c->d_pn, gamma_o, gamma_e);
            else
                hipLaunchKernelGGL((acx::qmax_path_kernel<false>), dim3(nb), dim3(64), 0, c->stream, dpd, c->d_pbox, c->d_bits, c->d_dir, c->d_pseam,
                                   c->d_pcells, c->d_pn, gamma_o, gamma_e);
        }
        ACX_HIP(c, hipGetLastError());
        h_n.resize((size_t)nb);
        h_cells.resize((size_t)(2 * ncell));
        ACX_HIP(c, hipMemcpyAsync(h_n.data(), c->d_pn, sizeof(int32_t) * nb, hipMemcpyDeviceToHost, c->stream));
        ACX_HIP(c, hipMemcpyAsync(h_cells.data(), c->d_pcells, sizeof(int32_t) * 2 * ncell, hipMemcpyDeviceToHost, c->stream));
        ACX_HIP(c, hipStreamSynchronize(c->stream));
        for (int b = 0; b < nb; ++b) {
            const acx::PathBox &bx = boxes[(size_t)b];
            const int n = h_n[(size_t)b];
            const int32_t *src = h_cells.data() + 2 * bx.cell_off;
            if (n < 1 || n > bx.max_cells || src[2 * (n - 1)] != bx.q0 || src[2 * (n - 1) + 1] != bx.r0)
                return fail(c, ACX_ERR_STATE, who + "the traceback of pair " + name(owner[(size_t)b]) + " does not end at the reported start");
            std::vector<int32_t> &out = dst(owner[(size_t)b]);
            out.resize((size_t)(2 * n));
            reverse_cells(src, n, out.data());
        }
    }
    drain_profile(c);
    return ACX_OK;
}

// The streaming class (a side beyond the last band class, or m > MAX_M) up to its recurrence bitmap, on the main stream: `B` pairs
// whose descriptors are `dpd` on the device and `pd` on the host, spanning `e`.
void launch_streaming_class(acx_ctx *c, const PairDesc *dpd, const PairDesc *pd, int B, const acx::Serra09Extent &e, const acx_serra09_params &p)
{
    {   // L1: D2 and D2^T
        const int tiles_x = (e.Mr + acx::LT - 1) / acx::LT, tiles_y = (e.Mq + acx::LT - 1) / acx::LT;
        ProfScope ps(c, KS_CSM, e.cells);
        hipLaunchKernelGGL(acx::csm_long_kernel, dim3(tiles_x * tiles_y, B), dim3(256), 0, c->stream,
                           c->active_frames(), c->active_toff(), dpd, c->d_scratch, tiles_x, p.oti_target, p.m);
    }
    {   // L2: thresholds of every row and column;  L3: recurrence bitmap
        int maxRows = 0;
        for (int k2 = 0; k2 < B; ++k2) maxRows = std::max(maxRows, pd[k2].Mq + pd[k2].Mr);
        ProfScope ps(c, KS_SEL, e.cells);
        hipLaunchKernelGGL(acx::rowsel_long_kernel, dim3((maxRows + 3) / 4, B), dim3(256), 0, c->stream,
                           dpd, c->d_scratch, c->d_thr, p.kappa, p.pct_mode, p.inclusive);
        hipLaunchKernelGGL(acx::binarise_long_kernel, dim3((e.Mq + 3) / 4, B), dim3(256), 0, c->stream,
                           dpd, c->d_scratch, c->d_thr, c->d_bits);
    }
}

// Runs the chain over `K` pairs in scratch-sized batches (behind run_serra09's guard, below).  `al` (acx_serra09_align): the sweep is
// qmax_locate_kernel and pair k's record goes to al[k]; no scores are written.  `paths` (acx_serra09_align_paths, with `al`; K vectors):
// the path pass runs behind the locating sweep of every batch, and pair k's cells go to (*paths)[k].  `al_dmax` (acx_chenfusion_align*,
// plane 1; with `al`): the locating sweep and the path pass are the Dmax ones.  `sec` (acx_serra09_align_sections, with `al`): the sweep is
// qmax_sections_kernel, pair k's sec->o.max_sections records go to al[k * max_sections ..] and their number to sec->n[k]; `paths` then
// has one vector per record.
int run_serra09_impl(acx_ctx *c, const int32_t *pairs, int64_t K, const acx_serra09_params &p_in, float *out,
                     const DebugOut *dbg, bool both, const DevDst *dd, acx_alignment *al, std::vector<std::vector<int32_t>> *paths, bool al_dmax,
                     const SectionRun *sec)
{
    const int per = sec ? sec->o.max_sections : 1;     // records per pair of an alignment run
    int32_t *const nsec = sec ? sec->n : nullptr;
    if (!c->d_frames0) return fail(c, ACX_ERR_STATE, "serra09: feature pool not uploaded (acx_upload_pool)");
    if (c->dim != acx::NBIN) return fail(c, ACX_ERR_INVALID, "serra09: pool dim must be 12");
    int rc = check_params(c, p_in);
    if (rc != ACX_OK) return rc;
    ACX_HIP(c, hipSetDevice(c->device));
    if ((rc = ensure_tau(c, p_in.tau)) != ACX_OK) return rc;
    acx_serra09_params p = p_in;
    p.tau = 1;                                   // from here on: the decimated pool
    const acx::Serra09Lengths len{c->h_off.data(), c->n_tracks, 1};
    const int64_t limit_floats = scratch_limit_bytes(c) / 4;
    constexpr int NC = acx::SERRA09_NC;          // band size classes; class NC: the streaming kernels
    const int w = both ? 2 : 1;
    if ((rc = validate_serra09_pairs(c, len, pairs, K, p, dbg != nullptr, limit_floats)) != ACX_OK) return rc;
    if (al) {      // the path start of a cell is ONE u32, row * Mr + column (the scratch limit refuses such a pair long before)
        PairDesc d;
        acx::Serra09Need need;
        for (int64_t k = 0; k < K; ++k) {
            (void)acx::serra09_size_pair(len, pairs[2 * k], pairs[2 * k + 1], p, false, d, need);
            if ((int64_t)d.Mq * d.Mr + acx::LOC_STRIP >= ((int64_t)1 << 32))      // (+ a strip: the wave indexes the columns right of the matrix too)
                return fail(c, ACX_ERR_UNSUPPORTED, std::string(al_dmax ? "chenfusion_align" : "serra09_align") + ": pair " + std::to_string(k) +
                                                        " has 2^32 cells or more");
        }
    }
    for (int s = 0; s < 2; ++s) {
        if (!c->slot[s].done) ACX_HIP(c, hipEventCreateWithFlags(&c->slot[s].done, hipEventDisableTiming));
        // (a slot is never marked free without its work being waited for: a failed call drains the streams, quiesce())
        if (c->slot[s].busy) { ACX_HIP(c, hipEventSynchronize(c->slot[s].done)); c->slot[s].busy = false; }
    }

    int64_t k0 = 0;
    for (int batch = 0; k0 < K; ++batch) {
        Serra09Slot &S = c->slot[batch & 1];
        if ((rc = collect_slot(c, S, out, al, nsec)) != ACX_OK) return rc;
        // the plan of the batch (serra09_plan.hpp): its pairs and their arena offsets, then the sort by size-class key --
        // `S.perm[k]` = position in the batch of sorted pair k
        std::vector<PairDesc> &pd = S.pd;
        acx::Serra09Arena used;
        const int64_t k = acx::serra09_pack_batch(len, pairs, k0, K, p, dbg != nullptr, limit_floats, pd, used);
        if (k == k0) return fail(c, ACX_ERR_STATE, "serra09: the batch plan made no progress at pair " + std::to_string(k0));
        const int B = (int)pd.size();
        const acx::Serra09Sort srt = acx::serra09_sort_batch(pd, S.sorted, S.perm, p.m);
        const int *key_begin = srt.key_begin, *cls_begin = srt.cls_begin;
        const std::vector<int> &perm = S.perm;
        if (cls_begin[NC] > 0 && (rc = ensure_normtab(c, p)) != ACX_OK) return rc;
        if (cls_begin[NC] > 0 && p.arith == ACX_ARITH_F16X2 && (rc = ensure_f16pool(c)) != ACX_OK) return rc;
        {   // a pass of the wide class (its row pass, or a column pass whose rows are of that class) in the exact arithmetic
            bool wide = cls_begin[NC] > cls_begin[NC - 1];
            for (int cl = 0; cl < NC; ++cl) wide = wide || key_begin[NC * cl + NC] > key_begin[NC * cl + NC - 1];
            if (wide && p.arith == ACX_ARITH_EXACT && (rc = ensure_planes(c)) != ACX_OK) return rc;
        }
        // (the band kernel reads its column thresholds 16 bytes at a time without a bounds check, up to
        // 64 x 32 floats behind a pair's column-threshold row: the arena carries that much slack)
        if ((rc = ensure(c, c->d_scratch, (size_t)std::max<int64_t>(used.scratch, 1))) != ACX_OK) return rc;
        if ((rc = ensure(c, c->d_bits, (size_t)std::max<int64_t>(used.bits, 1))) != ACX_OK) return rc;
        if ((rc = ensure(c, c->d_thr, (size_t)used.thr + 64 * 32 + 16)) != ACX_OK) return rc;
        if ((rc = ensure(c, S.d_pd, (size_t)B)) != ACX_OK) return rc;
        if ((rc = ensure(c, S.d_out, (size_t)2 * B)) != ACX_OK) return rc;
        if ((rc = ensure(c, S.h_out, (size_t)2 * B)) != ACX_OK) return rc;
        ACX_HIP(c, hipMemcpyAsync(S.d_pd, pd.data(), sizeof(PairDesc) * B, hipMemcpyHostToDevice, c->stream));
        if (al) {     // the locating sweep's records, and the seam records of the batch's pairs wider than one strip
            int64_t seams = 0;
            S.seam_off.resize((size_t)B);
            for (int k2 = 0; k2 < B; ++k2) { S.seam_off[(size_t)k2] = seams; seams += acx::loc_seam_records(pd[k2].Mq, pd[k2].Mr, p.dp_start); }
            if ((rc = ensure(c, S.d_al, (size_t)B * per)) != ACX_OK) return rc;
            if ((rc = ensure(c, S.h_al, (size_t)B * per)) != ACX_OK) return rc;
            if (sec && (rc = ensure(c, S.d_nsec, (size_t)B)) != ACX_OK) return rc;
            if (sec && (rc = ensure(c, S.h_nsec, (size_t)B)) != ACX_OK) return rc;
            if ((rc = ensure(c, S.d_seam_off, (size_t)B)) != ACX_OK) return rc;
            if ((rc = ensure(c, c->d_seam, (size_t)std::max<int64_t>(seams, 1))) != ACX_OK) return rc;
            ACX_HIP(c, hipMemcpyAsync(S.d_seam_off, S.seam_off.data(), sizeof(int64_t) * B, hipMemcpyHostToDevice, c->stream));
        }
        if (dd) {     // destinations of the batch's scores (staged here: the scatter may run on the second stream)
            if ((rc = ensure(c, S.h_idx, (size_t)B)) != ACX_OK) return rc;
            if ((rc = ensure(c, S.d_idx, (size_t)B)) != ACX_OK) return rc;
            for (int k2 = 0; k2 < B; ++k2) S.h_idx[k2] = dd->idx[k0 + perm[k2]];
            ACX_HIP(c, hipMemcpyAsync(S.d_idx, S.h_idx, sizeof(int64_t) * B, hipMemcpyHostToDevice, c->stream));
        }
        // The alignment sweeps are one wave per pair (or per two / four pairs) walking ~45 dependent packed instructions per matrix
        // row: a launch of a few thousand waves is bound by that chain's latency, not by the SIMDs (covers80-shaped call: four
        // launches, 1.16 of 8.8 ms; T = 2000: 0.92 ms per 2016 pairs at 2 waves per SIMD).  They go to a SECOND stream: the sweep of
        // size class cl starts when that class's bitmap is complete (cls_ev) and runs beside the band kernels of the next classes
        // and of the NEXT batch, whose row pass -- the writer of the shared bitmap arena -- waits for this batch's sweeps (S.done).
        // Not for batches with long pairs (their sweep's strip records live in the shared scratch), the debug entry point, or while
        // the per-kernel event clocks are on (acx_profile_enable: a kernel's time is then its time ALONE, not beside another launch).
        // (ACX_QMAX_STREAM=0 keeps them on the main stream.)
        // (nor for acx_serra09_align: one seam buffer serves both slots, and its lists are thousands of pairs, not millions)
        const bool use_q = acx::serra09_switches().qstream && !dbg && !al && !c->prof && cls_begin[NC + 1] == cls_begin[NC];
        if (use_q && !c->qstream) ACX_HIP(c, hipStreamCreateWithFlags(&c->qstream, hipStreamNonBlocking));
        if (use_q && both && !c->qstream2) {
            ACX_HIP(c, hipStreamCreateWithFlags(&c->qstream2, hipStreamNonBlocking));
            ACX_HIP(c, hipEventCreateWithFlags(&c->q2_done, hipEventDisableTiming));
        }
        hipStream_t qs = use_q ? c->qstream : c->stream;
        if (use_q)
            for (int cl = 0; cl < NC; ++cl)
                if (!S.cls_ev[cl]) ACX_HIP(c, hipEventCreateWithFlags(&S.cls_ev[cl], hipEventDisableTiming));
        Serra09Slot &Sprev = c->slot[(batch & 1) ^ 1];
        bool bits_free = !(Sprev.busy && Sprev.on_q);     // false: the previous batch's sweeps may still be reading the bitmap arena

        {   // K0
            ProfScope ps(c, KS_OTI, acx::serra09_extent(pd, 0, B).cells);
            hipLaunchKernelGGL(acx::oti_kernel, dim3((B + 255) / 256), dim3(256), 0, c->stream,
                               S.d_pd, B, c->d_gch, p.oti, p.oti_target, c->active_toff(), c->d_noff);
        }
        int64_t cls_cells[NC + 1];
        for (int cl = 0; cl <= NC; ++cl) {
            cls_cells[cl] = 0;
            const int b0 = cls_begin[cl], Bc = cls_begin[cl + 1] - b0;
            if (Bc <= 0) continue;
            const acx::Serra09Extent ce = acx::serra09_extent(pd, b0, b0 + Bc);
            cls_cells[cl] = ce.cells;
            if (cl < NC) {
                bool ok = true;
                // K1' role 1: rows = reference frames (Mq cells each) -> column thresholds; one launch per (cr, cq) key
                for (int cq = 0; cq < NC; ++cq) {
                    const int q0 = key_begin[NC * cl + cq], Bq = key_begin[NC * cl + cq + 1] - q0;
                    if (Bq <= 0) continue;
                    const acx::Serra09Extent qe = acx::serra09_extent(pd, q0, q0 + Bq);
                    ProfScope ps(c, KS_BAND, qe.cells);
                    ok = ok && launch_band(c, p.m, S.d_pd + q0, pd, q0, Bq, qe.Mr, cq, p, 1, 0, dbg ? 1 : 0);
                }
                if (!bits_free) { ACX_HIP(c, hipStreamWaitEvent(c->stream, Sprev.done, 0)); bits_free = true; }
                {   // K1' role 0: rows = query frames (Mr cells each) -> row thresholds + recurrence bitmap (needs role 1)
                    ProfScope ps(c, KS_BAND, ce.cells);
                    ok = ok && launch_band(c, p.m, S.d_pd + b0, pd, b0, Bc, ce.Mq, cl, p, 0, dbg ? 1 : 0, dbg ? 1 : 0);
                }
                if (use_q) ACX_HIP(c, hipEventRecord(S.cls_ev[cl], c->stream));
                if (!ok) return fail(c, ACX_ERR_UNSUPPORTED, "serra09: this build of libacx has no band kernel for the requested m");
            } else {
                if (!bits_free) { ACX_HIP(c, hipStreamWaitEvent(c->stream, Sprev.done, 0)); bits_free = true; }
                launch_streaming_class(c, S.d_pd + b0, &pd[b0], Bc, ce, p);
            }
        }
        {   // K3: one sweep per requested alignment over the SAME recurrence bitmap:
            // both == 0: Qmax or Dmax as p.dmax says; both == 1: out[2k] = Qmax, out[2k+1] = Dmax
            // one launch per size class, with the columns per lane and the pairs per wave of that class's row of the plan's table
            // (the default penalties' packed kernels take the two narrow classes four / two pairs per wave; ACX_QMAX_MULTI=0: one)
            hipError_t wait_err = hipSuccess;            // (a failed cross-stream wait would let a sweep read an unfinished bitmap: reported, not ignored)
            auto sweep = [&](bool dmax, float *dst, hipStream_t qs) {
                for (int cl = 0; cl <= NC; ++cl) {
                    const int b0 = cls_begin[cl], Bc = cls_begin[cl + 1] - b0;
                    if (Bc <= 0) continue;
                    if (use_q) { const hipError_t e_ = hipStreamWaitEvent(qs, S.cls_ev[cl], 0); if (e_ != hipSuccess) wait_err = e_; }
                    ProfScope ps(c, KS_QMAX, cls_cells[cl], qs);      // (its first event stands behind the wait)
                    const acx::Serra09Sweep sw = acx::serra09_sweep(cl);
                    launch_qmax_sweep(qs, S.d_pd + b0, Bc, c->d_bits, c->d_scratch, dst + (size_t)b0 * w, w, p.gamma_o, p.gamma_e, p.dp_start, dmax,
                                      sw.cols, sw.pack);
                }
            };
            if (sec) {                // every section: one launch for the batch, the loop over sections inside it
                ProfScope ps(c, KS_SECTIONS, acx::serra09_extent(pd, 0, B).cells, qs);
                launch_qmax_sections(qs, S.d_pd, B, c->d_bits, c->d_seam, S.d_seam_off, S.d_al, S.d_nsec, p.gamma_o, p.gamma_e, p.dp_start, sec->o);
            } else if (al) {          // WHERE the alignment lies: one launch for the batch, every class the same kernel
                ProfScope ps(c, al_dmax ? KS_DLOCATE : KS_LOCATE, acx::serra09_extent(pd, 0, B).cells, qs);
                if (al_dmax) launch_dmax_locate(qs, S.d_pd, B, c->d_bits, c->d_seam, S.d_seam_off, S.d_al, p.gamma_o, p.gamma_e, p.dp_start);
                else launch_qmax_locate(qs, S.d_pd, B, c->d_bits, c->d_seam, S.d_seam_off, S.d_al, p.gamma_o, p.gamma_e, p.dp_start);
            } else if (both && use_q) {      // the two alignments of a pair read the same bitmap and write different halves of d_out: side by side
                sweep(false, S.d_out, qs);
                sweep(true, S.d_out + 1, c->qstream2);
                ACX_HIP(c, hipEventRecord(c->q2_done, c->qstream2));
                ACX_HIP(c, hipStreamWaitEvent(qs, c->q2_done, 0));
            } else if (both) { sweep(false, S.d_out, qs); sweep(true, S.d_out + 1, qs); }
            else sweep(p.dmax != 0, S.d_out, qs);
            ACX_HIP(c, wait_err);
        }
        ACX_LAUNCHES_OK(c);
        if (al) {
            ACX_HIP(c, hipMemcpyAsync(S.h_al, S.d_al, sizeof(acx_alignment) * B * per, hipMemcpyDeviceToHost, qs));
            if (sec) ACX_HIP(c, hipMemcpyAsync(S.h_nsec, S.d_nsec, sizeof(int32_t) * B, hipMemcpyDeviceToHost, qs));
        } else if (dd) {
            hipLaunchKernelGGL(scatter_scores_kernel, dim3((B + 255) / 256), dim3(256), 0, qs,
                               S.d_out, S.d_idx, dd->base, B, w);
            ACX_HIP(c, hipGetLastError());
        } else {
            ACX_HIP(c, hipMemcpyAsync(S.h_out, S.d_out, sizeof(float) * B * w, hipMemcpyDeviceToHost, qs));
        }
        ACX_HIP(c, hipEventRecord(S.done, qs));
        S.busy = true; S.on_q = use_q; S.B = B; S.w = w; S.k0 = k0; S.al = al != nullptr; S.sec = sec ? per : 0;
        if (al && paths) {     // the paths, while d_bits holds this batch: the boxes come from the batch's records, so the host waits here
            ACX_HIP(c, hipEventSynchronize(S.done));
            if ((rc = run_qmax_paths(c, S.d_pd, S.h_al, B, p.gamma_o, p.gamma_e,
                                     [&](int k2) -> std::vector<int32_t> & { return (*paths)[(size_t)(k0 + perm[k2 / per]) * per + k2 % per]; },
                                     [&](int k2) { return std::to_string(k0 + perm[k2 / per]); }, al_dmax, per)) != ACX_OK) return rc;
        }

        if (dbg && B >= 1) {
            if ((rc = collect_slot(c, S, out)) != ACX_OK) return rc;
            PairDesc d;
            ACX_HIP(c, hipMemcpy(&d, S.d_pd, sizeof(PairDesc), hipMemcpyDeviceToHost));
            if (dbg->oti) *dbg->oti = d.oti;
            if (dbg->dims) { dbg->dims[0] = d.Mq; dbg->dims[1] = d.Mr; }
            if (dbg->d2)
                ACX_HIP(c, hipMemcpy2D(dbg->d2, sizeof(float) * d.Mr, c->d_scratch + d.offD, sizeof(float) * d.pitchD,
                                       sizeof(float) * d.Mr, d.Mq, hipMemcpyDeviceToHost));
            const float *X = c->d_thr + d.offX;
            if (dbg->thrq) ACX_HIP(c, hipMemcpy(dbg->thrq, X, sizeof(float) * d.Mq, hipMemcpyDeviceToHost));
            if (dbg->thrr) ACX_HIP(c, hipMemcpy(dbg->thrr, X + d.pitchT, sizeof(float) * d.Mr, hipMemcpyDeviceToHost));
            if (dbg->epsq) ACX_HIP(c, hipMemcpy(dbg->epsq, X + d.pitchT + d.pitchD, sizeof(float) * d.Mq, hipMemcpyDeviceToHost));
            if (dbg->epsr) ACX_HIP(c, hipMemcpy(dbg->epsr, X + 2 * d.pitchT + d.pitchD, sizeof(float) * d.Mr, hipMemcpyDeviceToHost));
        }
        k0 = k;
    }
    for (int s = 0; s < 2; ++s)
        if ((rc = collect_slot(c, c->slot[s], out, al, nsec)) != ACX_OK) return rc;
    return ACX_OK;
}

int run_serra09(acx_ctx *c, const int32_t *pairs, int64_t K, const acx_serra09_params &p_in, float *out,
                const DebugOut *dbg, bool both = false, const DevDst *dd = nullptr, acx_alignment *al = nullptr,
                std::vector<std::vector<int32_t>> *paths = nullptr, bool al_dmax = false, const SectionRun *sec = nullptr)
{
    return guarded(c, [&] { return run_serra09_impl(c, pairs, K, p_in, out, dbg, both, dd, al, paths, al_dmax, sec); });
}

}  // namespace


// ---------------------------------------------------------------------------------------
// EarlyFusion driver
// ---------------------------------------------------------------------------------------
// what the selection kernels left behind for one pair (acx_ef_debug_bits / acx_csm_debug_bits); any pointer may be null
struct EfStats { uint32_t *bits; float *t; int32_t *jcut; float *r; float *c; };
struct EfDebug { float *csm, *fused; int32_t *oti; int64_t which = 0; const EfStats *stats = nullptr; };      // which: the pair of the (one-batch) list whose intermediates are wanted

// acx_ef_align: what a run adds to the scores -- for every pair the record of ONE plane (0..3: mfccs, ssms, chromas, early) and,
// when `paths` is given (K vectors), the cells (q, r) of its path from start to end.  Pair k of the run's list -> al[k], (*paths)[k].
// any_length (acx_ef_align_long): a list with a track of more than 1024 blocks is not refused -- its batches take the float path, and
// ef_align_long_kernel reads the plot off the float matrices.
// sec (acx_ef_align_sections): EVERY section of a pair -- the batch's chunks run ef_sections_kernel in place of
// ef_align_kernel, pair k's sec->max_sections records go to al[k * max_sections ..], their number to n_sec[k] and, with `paths`
// (K * max_sections vectors), the cells of record t to (*paths)[t].  The bit path only.
struct EfAlign {
    int plane; acx_alignment *al; std::vector<std::vector<int32_t>> *paths; bool any_length;
    const acx_section_opts *sec = nullptr; int32_t *n_sec = nullptr;
};

// pinned host staging + device copy of `n` score destinations idx[0 .. n)
static int stage_idx(acx_ctx *c, const int64_t *idx, int64_t n)
{
    int rc;
    if ((rc = ensure(c, c->h_idx, (size_t)n)) != ACX_OK) return rc;
    if ((rc = ensure(c, c->d_idx, (size_t)n)) != ACX_OK) return rc;
    memcpy(c->h_idx, idx, sizeof(int64_t) * (size_t)n);
    ACX_HIP(c, hipMemcpyAsync(c->d_idx, c->h_idx, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    return ACX_OK;
}

// Rectangles for the segment GEMM: consecutive pairs of the batch are collected while they involve at most
// SEG_TRACKS distinct query and SEG_TRACKS distinct reference tracks (and no (query, reference) combination
// twice); the blocks of those tracks, each padded to a multiple of 16, become the rows / columns of one dense
// matrix.  A grid tile of 128 x 128 tracks is exactly one rectangle; an arbitrary pair list degrades to
// rectangles whose pair table is mostly -1 (their empty workgroup tiles return at once).
static int ef_build_splits(acx_ctx *c, int fmt);
namespace {
constexpr int SEG_TRACKS = 128;
struct SegBatch {
    std::vector<acx::EfSegGroup> rowg, colg;
    std::vector<acx::EfSegRect> rects;
    std::vector<int32_t> ptab;
    std::vector<acx::EfSegWg> wgs;          // workgroup tiles of 8 x 8 groups (128 x 128 cells: ef_gemm_seg_f32_kernel)
    std::vector<acx::EfSegWg> wgs2;         // tiles of 16 x 8 groups (256 x 128 cells: ef_gemm_rect_bf16x3_kernel<0>): ty, first column group, groups
    std::vector<acx::EfSegWg> wgs3;         // the same for chroma (<1>): the columns of a tile stop at the end of their reference track
};
void ef_build_rects(const std::vector<acx::EfPair> &pd, const std::vector<int64_t> &efoff, int n_tracks, SegBatch &sb,
                    std::vector<int32_t> &qslot, std::vector<int32_t> &rslot)
{
    sb.rowg.clear(); sb.colg.clear(); sb.rects.clear(); sb.ptab.clear(); sb.wgs.clear(); sb.wgs2.clear(); sb.wgs3.clear();
    std::vector<uint8_t> mark, mark2, mark3;
    std::vector<int32_t> cfirst;                  // chroma: first column chunk of every reference slot (+ one past the last)
    std::vector<std::pair<int32_t, int32_t>> cchunk;     // (first group, groups) of every column chunk
    std::vector<int32_t> gfirst_q, gfirst_r;      // first group of every slot (+ one past the last)
    qslot.assign((size_t)n_tracks, -1);
    rslot.assign((size_t)n_tracks, -1);
    std::vector<int32_t> qs, rs;                 // tracks of the open rectangle, in slot order
    std::vector<std::pair<int32_t, int32_t>> members;     // (pair index, qslot * SEG_TRACKS + rslot)
    std::vector<uint8_t> seen((size_t)SEG_TRACKS * SEG_TRACKS, 0);
    auto close = [&]() {
        if (members.empty()) return;
        acx::EfSegRect R;
        R.g0 = (int32_t)sb.rowg.size(); R.h0 = (int32_t)sb.colg.size();
        // a sparse rectangle (an arbitrary pair list: few of its query x reference combinations are pairs) starts every
        // track on a workgroup-tile boundary (8 groups), so that a tile never stages the rows of tracks it has no pair
        // for; a dense one (a grid tile) packs the tracks tightly: its tiles are full anyway
        const bool sparse = 2 * members.size() < qs.size() * rs.size();
        auto lay = [&](const std::vector<int32_t> &tracks, std::vector<acx::EfSegGroup> &out, std::vector<int32_t> &gfirst) {
            const size_t start = out.size();
            gfirst.clear();
            for (size_t sl = 0; sl < tracks.size(); ++sl) {
                while (sparse && ((out.size() - start) & 7) != 0) out.push_back(acx::EfSegGroup{0, 0, (int32_t)sl, 0, 0});
                gfirst.push_back((int32_t)(out.size() - start));
                const int64_t base = efoff[tracks[sl]];
                const int n = (int)(efoff[tracks[sl] + 1] - base);
                for (int l0 = 0; l0 < n; l0 += 16)
                    out.push_back(acx::EfSegGroup{base + l0, std::min(16, n - l0), (int32_t)sl, l0, 0});
            }
            gfirst.push_back((int32_t)(out.size() - start));
        };
        lay(qs, sb.rowg, gfirst_q);
        lay(rs, sb.colg, gfirst_r);
        R.ng = (int32_t)sb.rowg.size() - R.g0; R.nh = (int32_t)sb.colg.size() - R.h0;
        R.ncols = (int32_t)rs.size();
        R.ptab0 = (int32_t)sb.ptab.size();
        sb.ptab.resize(sb.ptab.size() + qs.size() * rs.size(), -1);
        // workgroup tiles (8 x 8 groups) that hold at least one pair, row-major: neighbours share their row operand
        const int tiles_y = (R.ng + 7) / 8, tiles_x = (R.nh + 7) / 8;
        const int tiles_y2 = (R.ng + 15) / 16;
        mark.assign((size_t)tiles_y * tiles_x, 0);
        mark2.assign((size_t)tiles_y2 * tiles_x, 0);
        cfirst.clear(); cchunk.clear();
        for (size_t sl = 0; sl < rs.size(); ++sl) {
            cfirst.push_back((int32_t)cchunk.size());
            for (int g = gfirst_r[sl]; g < gfirst_r[sl + 1]; g += 8) cchunk.push_back({g, std::min(8, gfirst_r[sl + 1] - g)});
        }
        cfirst.push_back((int32_t)cchunk.size());
        const int ncc = (int)cchunk.size();
        mark3.assign((size_t)tiles_y2 * ncc, 0);
        for (const auto &m : members) {
            const int a = m.second / SEG_TRACKS, b = m.second % SEG_TRACKS;
            sb.ptab[(size_t)R.ptab0 + (size_t)a * R.ncols + b] = m.first;
            seen[(size_t)m.second] = 0;
            if (gfirst_q[a + 1] == gfirst_q[a] || gfirst_r[b + 1] == gfirst_r[b]) continue;     // (a track without blocks)
            for (int ty = gfirst_q[a] / 8; ty <= (gfirst_q[a + 1] - 1) / 8; ++ty)
                for (int tx = gfirst_r[b] / 8; tx <= (gfirst_r[b + 1] - 1) / 8; ++tx) {
                    mark[(size_t)ty * tiles_x + tx] = 1;
                    mark2[(size_t)(ty / 2) * tiles_x + tx] = 1;
                }
            for (int ty = gfirst_q[a] / 16; ty <= (gfirst_q[a + 1] - 1) / 16; ++ty)
                for (int ci = cfirst[b]; ci < cfirst[b + 1]; ++ci) mark3[(size_t)ty * ncc + ci] = 1;
        }
        const int32_t rid = (int32_t)sb.rects.size();
        for (int ty = 0; ty < tiles_y; ++ty)
            for (int tx = 0; tx < tiles_x; ++tx)
                if (mark[(size_t)ty * tiles_x + tx]) sb.wgs.push_back(acx::EfSegWg{rid, ty, tx, 0});
        for (int ty = 0; ty < tiles_y2; ++ty)
            for (int tx = 0; tx < tiles_x; ++tx)
                if (mark2[(size_t)ty * tiles_x + tx]) sb.wgs2.push_back(acx::EfSegWg{rid, ty, 8 * tx, std::min(8, R.nh - 8 * tx)});
        for (int ty = 0; ty < tiles_y2; ++ty)
            for (int ci = 0; ci < ncc; ++ci)
                if (mark3[(size_t)ty * ncc + ci]) sb.wgs3.push_back(acx::EfSegWg{rid, ty, cchunk[(size_t)ci].first, cchunk[(size_t)ci].second});
        sb.rects.push_back(R);
        for (int32_t t : qs) qslot[(size_t)t] = -1;
        for (int32_t t : rs) rslot[(size_t)t] = -1;
        qs.clear(); rs.clear(); members.clear();
    };
    for (size_t k = 0; k < pd.size(); ++k) {
        const int q = pd[k].q, r = pd[k].r;
        for (int attempt = 0; attempt < 2; ++attempt) {
            const bool newq = qslot[(size_t)q] < 0, newr = rslot[(size_t)r] < 0;
            const bool fits = (!newq || (int)qs.size() < SEG_TRACKS) && (!newr || (int)rs.size() < SEG_TRACKS);
            const bool dup = !newq && !newr && seen[(size_t)qslot[(size_t)q] * SEG_TRACKS + rslot[(size_t)r]];
            if (fits && !dup) {
                if (newq) { qslot[(size_t)q] = (int32_t)qs.size(); qs.push_back(q); }
                if (newr) { rslot[(size_t)r] = (int32_t)rs.size(); rs.push_back(r); }
                const int code = qslot[(size_t)q] * SEG_TRACKS + rslot[(size_t)r];
                seen[(size_t)code] = 1;
                members.push_back({(int32_t)k, code});
                break;
            }
            close();                              // (the second attempt always fits an empty rectangle)
        }
    }
    close();
}
}  // namespace

// The three cross-similarity GEMMs of one batch into its scratch: mfcc and ssm (squared Euclidean distances, z = 0 / 1) and chroma
// (cosine, the first song rolled by the pair's OTI, z = 2).  One kernel path per mode:
//   ACX_EF_GEMM_F16X2 (default)   ef_gemm_rect_persist_dma_kernel<0 / 1>: one workgroup per CU walks the tiles, operands by LDS-DMA;
//                                 ACX_EF_PERSIST=0: ef_gemm_rect_bf16x3_kernel<0 / 1, 1>, one workgroup per tile -- the same bits, kept
//                                 as an independent cross-check of the DMA kernel
//   ACX_EF_GEMM_BF16X3            ef_gemm_rect_bf16x3_kernel<0 / 1, 0>
//   ACX_EF_GEMM_BF16X3_CHROMA_F32 ef_gemm_rect_bf16x3_kernel<0, 0>; chroma: ef_gemm_seg_f32_kernel (f32 MFMAs; so is every rectangle
//                                 mode's chroma when the split does not cover the block shape, ef_kp[2] == 0)
//   ACX_EF_GEMM_BF16X3_PAIRWISE   ef_gemm_bf16x3_kernel, one pair per grid row; chroma: ef_gemm_kernel
//   ACX_EF_GEMM_F32               ef_gemm_kernel
static int launch_ef_gemms(acx_ctx *c, const SegBatch &seg, int B, int tiles_x, int tiles_y)
{
    int rc;
    const bool f16 = c->ef_gemm == ACX_EF_GEMM_F16X2;
    if (c->ef_gemm != ACX_EF_GEMM_F32 && c->ef_split_fmt != (f16 ? 1 : 0))
        if ((rc = ef_build_splits(c, f16 ? 1 : 0)) != ACX_OK) return rc;
    if (c->ef_gemm == ACX_EF_GEMM_F32) {
        hipLaunchKernelGGL(acx::ef_gemm_kernel, dim3(tiles_x * tiles_y, B, 3), dim3(256), 0, c->stream,
                           c->d_ef[0], c->d_ef[1], c->d_ef[2], c->d_efn[0], c->d_efn[1], c->d_efoff, c->d_efpd,
                           c->d_scratch, c->ef_dims[0], c->ef_dims[1], c->ef_dims[2], tiles_x, 0);
        return ACX_OK;
    }
    if (c->ef_gemm == ACX_EF_GEMM_BF16X3_PAIRWISE) {
        hipLaunchKernelGGL(acx::ef_gemm_bf16x3_kernel, dim3(tiles_x * tiles_y, B, 2), dim3(acx::EFB_THREADS), 0, c->stream,
                           c->d_efs[0], c->d_efs[1], c->d_efn[0], c->d_efn[1], c->d_efoff, c->d_efpd,
                           c->d_scratch, c->ef_kp[0], c->ef_kp[1], tiles_x);
        hipLaunchKernelGGL(acx::ef_gemm_kernel, dim3(tiles_x * tiles_y, B, 1), dim3(256), 0, c->stream,
                           c->d_ef[0], c->d_ef[1], c->d_ef[2], c->d_efn[0], c->d_efn[1], c->d_efoff, c->d_efpd,
                           c->d_scratch, c->ef_dims[0], c->ef_dims[1], c->ef_dims[2], tiles_x, 2);
        return ACX_OK;
    }
    // the rectangle modes: the batch's rectangles to the device (the copies are staged before they return: `seg` may be rebuilt
    // for the next batch)
    if ((rc = ensure(c, c->d_segr, seg.rowg.size())) != ACX_OK) return rc;
    if ((rc = ensure(c, c->d_segc, seg.colg.size())) != ACX_OK) return rc;
    if ((rc = ensure(c, c->d_rects, seg.rects.size())) != ACX_OK) return rc;
    if ((rc = ensure(c, c->d_ptab, seg.ptab.size())) != ACX_OK) return rc;
    ACX_HIP(c, hipMemcpyAsync(c->d_segr, seg.rowg.data(), sizeof(acx::EfSegGroup) * seg.rowg.size(), hipMemcpyHostToDevice, c->stream));
    ACX_HIP(c, hipMemcpyAsync(c->d_segc, seg.colg.data(), sizeof(acx::EfSegGroup) * seg.colg.size(), hipMemcpyHostToDevice, c->stream));
    ACX_HIP(c, hipMemcpyAsync(c->d_rects, seg.rects.data(), sizeof(acx::EfSegRect) * seg.rects.size(), hipMemcpyHostToDevice, c->stream));
    ACX_HIP(c, hipMemcpyAsync(c->d_ptab, seg.ptab.data(), sizeof(int32_t) * seg.ptab.size(), hipMemcpyHostToDevice, c->stream));
    if (seg.wgs.size() > 0x7fffffffu || seg.wgs3.size() > 0x7fffffffu)
        return fail(c, ACX_ERR_UNSUPPORTED, "earlyfusion: batch too large for one launch");
    if (!c->ef_rect_attr) {
        for (const void *k : {reinterpret_cast<const void *>(acx::ef_gemm_rect_bf16x3_kernel<0, 0>),
                              reinterpret_cast<const void *>(acx::ef_gemm_rect_bf16x3_kernel<1, 0>),
                              reinterpret_cast<const void *>(acx::ef_gemm_rect_bf16x3_kernel<0, 1>),
                              reinterpret_cast<const void *>(acx::ef_gemm_rect_bf16x3_kernel<1, 1>),
                              reinterpret_cast<const void *>(acx::ef_gemm_rect_persist_dma_kernel<0>),
                              reinterpret_cast<const void *>(acx::ef_gemm_rect_persist_dma_kernel<1>)})
            ACX_HIP(c, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, acx::EFR_LDS_BYTES));
        if ((rc = ensure(c, c->d_efctr, 2)) != ACX_OK) return rc;
        c->ef_rect_attr = true;
    }
    // a list of workgroup tiles to the device
    auto upload = [c](const std::vector<acx::EfSegWg> &w, DeviceBuffer<acx::EfSegWg> &d) -> int {
        const int rc = ensure(c, d, w.size());
        if (rc != ACX_OK) return rc;
        ACX_HIP(c, hipMemcpyAsync(d, w.data(), sizeof(acx::EfSegWg) * w.size(), hipMemcpyHostToDevice, c->stream));
        return ACX_OK;
    };
    using RectKernel = decltype(&acx::ef_gemm_rect_bf16x3_kernel<0, 0>);
    // one workgroup per tile: mfcc and ssm over the 256 x 128-cell tiles of wgs2, chroma over those of wgs3 (their columns stop at
    // the end of their reference track)
    auto rect_eucl = [&](RectKernel kern) -> int {
        if (seg.wgs2.empty()) return ACX_OK;
        if ((rc = upload(seg.wgs2, c->d_segw2)) != ACX_OK) return rc;
        hipLaunchKernelGGL(kern, dim3((unsigned)seg.wgs2.size(), 1, 2), dim3(acx::EFR_THREADS), acx::EFR_LDS_BYTES, c->stream,
                           c->d_efs[0], c->d_efs[1], c->d_efn[0], c->d_efn[1], c->d_efpd, c->d_rects, c->d_segw2, c->d_segr, c->d_segc,
                           c->d_ptab, c->d_scratch, c->ef_kp[0], c->ef_kp[1], c->d_efsc[0], c->d_efsc[1]);
        return ACX_OK;
    };
    auto rect_chroma = [&](RectKernel kern) -> int {
        if (seg.wgs3.empty()) return ACX_OK;
        if ((rc = upload(seg.wgs3, c->d_segw3)) != ACX_OK) return rc;
        hipLaunchKernelGGL(kern, dim3((unsigned)seg.wgs3.size(), 1, 1), dim3(acx::EFR_THREADS), acx::EFR_LDS_BYTES, c->stream,
                           c->d_efs[2], c->d_efs[2], (const float *)nullptr, (const float *)nullptr, c->d_efpd, c->d_rects, c->d_segw3,
                           c->d_segr, c->d_segc, c->d_ptab, c->d_scratch, c->ef_kp[2], c->ef_kp[2], c->d_efsc[2], c->d_efsc[2]);
        return ACX_OK;
    };
    // chroma on f32 MFMAs over the 128 x 128-cell tiles of wgs
    auto f32_chroma = [&]() -> int {
        if (seg.wgs.empty()) return ACX_OK;
        if ((rc = upload(seg.wgs, c->d_segw)) != ACX_OK) return rc;
        hipLaunchKernelGGL(acx::ef_gemm_seg_f32_kernel, dim3((unsigned)seg.wgs.size()), dim3(256), 0, c->stream,
                           c->d_ef[2], c->d_efpd, c->d_rects, c->d_segw, c->d_segr, c->d_segc, c->d_ptab, c->d_scratch, c->ef_dims[2]);
        return ACX_OK;
    };
    const bool chroma_split = c->ef_kp[2] > 0;
    static const bool one_tile = [] { const char *e = getenv("ACX_EF_PERSIST"); return e && e[0] == '0'; }();
    if (f16 && !one_tile) {
        // one workgroup per CU, each walking the tiles that the counters d_efctr[0] (mfcc, ssm) and [1] (chroma) deal out
        const int ncu = std::max(1, c->n_cu);
        if (!seg.wgs2.empty()) {
            if ((rc = upload(seg.wgs2, c->d_segw2)) != ACX_OK) return rc;
            const int nt = (int)seg.wgs2.size();
            const unsigned grid = (unsigned)std::min<int64_t>(ncu, 2 * (int64_t)nt);
            ACX_HIP(c, hipMemsetD32Async((hipDeviceptr_t)c->d_efctr, (int)(2 * grid), 1, c->stream));
            hipLaunchKernelGGL(acx::ef_gemm_rect_persist_dma_kernel<0>, dim3(grid), dim3(acx::EFR_THREADS), acx::EFR_LDS_BYTES, c->stream,
                               c->d_efs[0], c->d_efs[1], c->d_efn[0], c->d_efn[1], c->d_efpd, c->d_rects, c->d_segw2, c->d_segr,
                               c->d_segc, c->d_ptab, c->d_scratch, c->ef_kp[0], c->ef_kp[1], c->d_efsc[0], c->d_efsc[1], nt, 2, c->d_efctr);
        }
        if (!chroma_split) return f32_chroma();
        if (!seg.wgs3.empty()) {
            if ((rc = upload(seg.wgs3, c->d_segw3)) != ACX_OK) return rc;
            const int nt = (int)seg.wgs3.size();
            const unsigned grid = (unsigned)std::min(ncu, nt);
            ACX_HIP(c, hipMemsetD32Async((hipDeviceptr_t)(c->d_efctr + 1), (int)(2 * grid), 1, c->stream));
            hipLaunchKernelGGL(acx::ef_gemm_rect_persist_dma_kernel<1>, dim3(grid), dim3(acx::EFR_THREADS), acx::EFR_LDS_BYTES, c->stream,
                               c->d_efs[2], c->d_efs[2], (const float *)nullptr, (const float *)nullptr, c->d_efpd, c->d_rects,
                               c->d_segw3, c->d_segr, c->d_segc, c->d_ptab, c->d_scratch, c->ef_kp[2], c->ef_kp[2],
                               c->d_efsc[2], c->d_efsc[2], nt, 1, c->d_efctr + 1);
        }
        return ACX_OK;
    }
    if (f16) {
        if ((rc = rect_eucl(acx::ef_gemm_rect_bf16x3_kernel<0, 1>)) != ACX_OK) return rc;
        return chroma_split ? rect_chroma(acx::ef_gemm_rect_bf16x3_kernel<1, 1>) : f32_chroma();
    }
    if (c->ef_gemm == ACX_EF_GEMM_BF16X3) {
        if ((rc = rect_eucl(acx::ef_gemm_rect_bf16x3_kernel<0, 0>)) != ACX_OK) return rc;
        return chroma_split ? rect_chroma(acx::ef_gemm_rect_bf16x3_kernel<1, 0>) : f32_chroma();
    }
    // ACX_EF_GEMM_BF16X3_CHROMA_F32
    if ((rc = rect_eucl(acx::ef_gemm_rect_bf16x3_kernel<0, 0>)) != ACX_OK) return rc;
    return f32_chroma();
}

// One pair of M x N at offset 0 of every arena: a caller's matrix or plot as a batch of its own.
static acx::EfPair ef_one_pair(int M, int N, int kbin = 0)
{
    acx::EfPair d = acx::ef_pair_desc(0, 0, M, N, 1.0, false);
    d.kbin = kbin;                        // (the caller's, not a kappa's)
    return d;
}

// One job's result of ef_align_kernel / ef_align_long_kernel on the host: `rec` its EFA_REC words, `src` its cells as the traceback left
// them, read only where `path` is given; the record goes to `out`, the cells from the start to the end to `path`.  The errors read
// who + ": the traceback" + of + ...; `score` (or nullptr): the bits the record's score must have.
static int decode_ef_alignment(acx_ctx *c, const std::string &who, const std::string &of, const int32_t *rec, const int32_t *src, int max_cells,
                               const float *score, acx_alignment &out, std::vector<int32_t> *path)
{
    acx_alignment a;
    memcpy(&a.score, rec, sizeof(float));
    a.q0 = rec[1]; a.r0 = rec[2]; a.q1 = rec[3]; a.r1 = rec[4];
    const int n = rec[5];
    // the score is the one the batch's Smith-Waterman launch left for this pair and plane, and a match has its cells
    if (score && memcmp(&a.score, score, sizeof(float)) != 0)
        return fail(c, ACX_ERR_STATE, who + ": the alignment" + of + " does not reach the pair's score");
    if (n < 0 || n > max_cells || (a.score > 0.0f) != (n >= 1))
        return fail(c, ACX_ERR_STATE, who + ": the traceback" + of + " returned " + std::to_string(n) + " cells");
    out = a;
    if (!path) return ACX_OK;
    if (n >= 1 && (src[0] != a.q1 || src[1] != a.r1 || src[2 * (n - 1)] != a.q0 || src[2 * (n - 1) + 1] != a.r0))
        return fail(c, ACX_ERR_STATE, who + ": the traceback" + of + " does not run from the reported end to the reported start");
    path->resize(2 * (size_t)n);
    reverse_cells(src, n, path->data());
    return ACX_OK;
}

// One job's result of ef_sections_kernel on the host: `n` its number of sections, `rec` its S records of EFA_REC
// words, `src` its cells -- the sections' behind one another, each as the traceback left it -- read only where `paths` (S vectors) is
// given, `room` what the job had for them.  Every section goes through decode_ef_alignment: section 0 must have the bits of `score`
// (or nullptr), every section its cells from the reported end to the reported start.  Beyond that: the count is within S, the
// records behind it are the no-match record, scores do not increase, and the row ranges are pairwise disjoint.
static int decode_ef_sections(acx_ctx *c, const std::string &who, const std::string &of, int S, int n, const int32_t *rec, const int32_t *src,
                              int64_t room, int side, const float *score, float min_score, acx_alignment *out, int32_t &n_out,
                              std::vector<int32_t> *paths)
{
    if (n < 0 || n > S) return fail(c, ACX_ERR_STATE, who + ": the sections" + of + " number " + std::to_string(n));
    const float zero = 0.0f;
    int64_t used = 0;
    for (int s = 0; s < S; ++s) {
        const int32_t *r = rec + (size_t)acx::EFA_REC * s;
        const int ns = r[5];
        if (ns < 0 || used + ns > room) return fail(c, ACX_ERR_STATE, who + ": the traceback" + of + " returned " + std::to_string(ns) + " cells");
        // a pair whose alignment stays below min_score has no sections: section 0's score is then not the kernel's to report
        const float *want = s == 0 && n > 0 ? score : (s >= n ? &zero : nullptr);
        int rc = decode_ef_alignment(c, who, of, r, src ? src + 2 * used : nullptr, side, want, out[s], paths ? &paths[s] : nullptr);
        if (rc != ACX_OK) return rc;
        used += ns;
        if (s < n) {
            if (!(out[s].score > 0.0f) || (s > 0 && out[s].score > out[s - 1].score))
                return fail(c, ACX_ERR_STATE, who + ": the scores of the sections" + of + " are not in order");
            for (int t = 0; t < s; ++t)
                if (out[s].q0 <= out[t].q1 && out[t].q0 <= out[s].q1)
                    return fail(c, ACX_ERR_STATE, who + ": sections " + std::to_string(t) + " and " + std::to_string(s) + of + " share a row");
        }
    }
    if (n == 0 && score && *score >= min_score)
        return fail(c, ACX_ERR_STATE, who + ": no section" + of + " although the pair's score reaches min_score");
    n_out = n;
    return ACX_OK;
}

// The alignment pass (ef_align_kernels.hpp) behind a batch's Smith-Waterman launch, while d_efbits and d_efpd
// still hold the batch: `pd` are the batch's descriptors on the host, pair b of the batch is pair k0 + b of the run, `scores` its
// four scores (queued behind the batch's kernels: valid after a wait).  The batch's pairs run in CHUNKS: as many consecutive pairs
// as fit `budget` bytes of direction planes (M * pitch / 4 bytes a pair; the first pair of a chunk is always taken -- a pair's
// plane is 1 / 48 of the three float matrices the same pair holds in the batch, so it fits half of any limit the batch fits) and
// one launch's grid; one launch, one copy and one wait per chunk.  Returns with the stream idle.
static int64_t ef_align_wave_cap()
{
    // development aid (ACX_EF_ALIGN_WAVES=n, read per call): fewer waves per chunk than a launch's 65535, so that a short list runs
    // in several chunks
    const char *e = getenv("ACX_EF_ALIGN_WAVES");
    const long v = e ? atol(e) : 0;
    return v >= 1 && v < 65535 ? v : 65535;
}

// What run_ef_align_jobs launches: ef_align_long_kernel (`float_path`), ef_sections_kernel (`sec`) or ef_align_kernel, on `plane`.
// `cells`: the jobs' cells come back behind the records.  `prof_area` >= 0: a profile scope of that many cells (the caller drains).
struct EfAlignLaunch {
    bool float_path; int plane; const acx_section_opts *sec; bool cells; int64_t prof_area;
};

// words of nb jobs' records in a result block, in front of the cells (sections: the counts, then S records a job)
static size_t ef_align_nrec(int nb, int S) { return S ? (size_t)nb + (size_t)acx::EFA_REC * S * nb : (size_t)acx::EFA_REC * nb; }

// One launch over `jobs`, whose pairs d_efpd holds and whose direction planes take `words` u32 in all: ensures d_efdir, d_efjob and
// d_efres, copies the jobs, launches, brings the result block back into `h_res`, and waits.
static int run_ef_align_jobs(acx_ctx *c, const std::vector<acx::EfAlignJob> &jobs, int64_t words, const EfAlignLaunch &L, std::vector<int32_t> &h_res)
{
    const int nb = (int)jobs.size(), S = L.sec ? L.sec->max_sections : 0;
    const size_t nrec = ef_align_nrec(nb, S), nres = nrec + 2 * (size_t)(jobs.back().cell_off + jobs.back().max_cells);
    int rc;
    if ((rc = ensure(c, c->d_efdir, (size_t)words)) != ACX_OK) return rc;
    if ((rc = ensure(c, c->d_efjob, (size_t)nb)) != ACX_OK) return rc;
    if ((rc = ensure(c, c->d_efres, nres)) != ACX_OK) return rc;
    ACX_HIP(c, hipMemcpyAsync(c->d_efjob, jobs.data(), sizeof(acx::EfAlignJob) * nb, hipMemcpyHostToDevice, c->stream));
    {
        std::optional<ProfScope> ps;
        if (L.prof_area >= 0) ps.emplace(c, L.float_path ? KS_EFALIGNLONG : (S ? KS_EFSECTIONS : KS_EFALIGN), L.prof_area);
        if (L.float_path)       // (no bitmaps: the plot from the float matrices, thresholds and tie columns; the record areas are free by now)
            hipLaunchKernelGGL(acx::ef_align_long_kernel, dim3(nb), dim3(64), 0, c->stream, c->d_efpd, c->d_efjob, c->d_scratch, c->d_thr, c->d_efdir, c->d_efres, L.plane);
        else if (S)
            hipLaunchKernelGGL(acx::ef_sections_kernel, dim3(nb), dim3(64), 0, c->stream, c->d_efpd, c->d_efjob, c->d_efbits, c->d_efdir, c->d_efres, L.plane,
                               S, L.sec->pad, L.sec->min_score, L.sec->min_ratio);
        else
            hipLaunchKernelGGL(acx::ef_align_kernel, dim3(nb), dim3(64), 0, c->stream, c->d_efpd, c->d_efjob, c->d_efbits, c->d_efdir, c->d_efres, L.plane);
    }
    ACX_HIP(c, hipGetLastError());
    h_res.resize(L.cells ? nres : nrec);                             // (records and counts alone when no path is wanted)
    ACX_HIP(c, hipMemcpyAsync(h_res.data(), c->d_efres, sizeof(int32_t) * h_res.size(), hipMemcpyDeviceToHost, c->stream));
    ACX_HIP(c, hipStreamSynchronize(c->stream));
    return ACX_OK;
}

static int run_ef_align_batch(acx_ctx *c, const std::vector<acx::EfPair> &pd, int64_t k0, int64_t budget, const EfAlign &aln, const float *scores,
                              bool float_path)
{
    const int B = (int)pd.size();
    const int64_t wave_cap = ef_align_wave_cap();
    const int S = aln.sec ? aln.sec->max_sections : 0;              // > 0: every section of a pair (ef_sections_kernel)
    std::vector<acx::EfAlignJob> jobs;
    std::vector<int32_t> h_res;
    int b = 0;
    while (b < B) {
        jobs.clear();
        int64_t words = 0, ncell = 0, area = 0;
        const int b0 = b;
        for (; b < B && (int64_t)jobs.size() < wave_cap; ++b) {
            const acx::EfPair &d = pd[(size_t)b];
            const int64_t w = float_path ? acx::ef_align_long_dir_words(d.M, d.N) : acx::ef_align_dir_words(d.M, d.pitchC);
            if (!jobs.empty() && 4 * (words + w) > budget) break;
            acx::EfAlignJob j;
            // (sections: the room of ALL the pair's sections, ef_sections_room)
            j.pair = b; j.max_cells = S ? (int)acx::ef_sections_room(d.M, d.N, S) : std::min(d.M, d.N); j.dir_off = words; j.cell_off = ncell;
            words += w;
            ncell += j.max_cells;
            area += (int64_t)d.M * d.N;
            jobs.push_back(j);
        }
        const int nb = (int)jobs.size();
        const size_t nrec = ef_align_nrec(nb, S);
        int rc;
        if ((rc = run_ef_align_jobs(c, jobs, words, {float_path, aln.plane, aln.sec, aln.paths != nullptr, area}, h_res)) != ACX_OK) return rc;
        for (int t = 0; t < nb; ++t) {
            const acx::EfAlignJob &j = jobs[(size_t)t];
            const int64_t k = k0 + b0 + t;
            const int32_t *src = aln.paths ? h_res.data() + nrec + 2 * (size_t)j.cell_off : nullptr;
            if (S) {
                const acx::EfPair &d = pd[(size_t)j.pair];
                if ((rc = decode_ef_sections(c, "ef_align_sections", " of pair " + std::to_string(k), S, h_res[(size_t)t],
                                             h_res.data() + nb + (size_t)acx::EFA_REC * S * t, src, j.max_cells, std::min(d.M, d.N),
                                             scores + 4 * (size_t)(b0 + t) + aln.plane, aln.sec->min_score, aln.al + (size_t)k * S, aln.n_sec[k],
                                             aln.paths ? &(*aln.paths)[(size_t)k * S] : nullptr)) != ACX_OK)
                    return rc;
                continue;
            }
            if ((rc = decode_ef_alignment(c, "ef_align", " of pair " + std::to_string(k), h_res.data() + (size_t)acx::EFA_REC * t, src, j.max_cells,
                                          scores + 4 * (size_t)(b0 + t) + aln.plane, aln.al[k], aln.paths ? &(*aln.paths)[(size_t)k] : nullptr)) != ACX_OK)
                return rc;
        }
    }
    drain_profile(c);
    return ACX_OK;
}

// One batch on the host: its pair descriptors and arena extents (ef_pack_batch, ef_plan.hpp) and -- for the rectangle GEMM -- the
// dense rectangles its pairs are laid out in.  Built for batch b + 1 WHILE the device works on batch b (two of these; the copies to
// the device are staged before they return): ~1 ms per 16 384 pairs that the device used to wait for between batches.
struct EfHostBatch {
    std::vector<acx::EfPair> pd;
    SegBatch seg;
    std::vector<int32_t> qslot, rslot;          // (ef_build_rects' own)
    int64_t k_begin = 0, k_end = 0;
    acx::EfArena a;
};

// what run_ef_impl has settled about a checked list before its first batch
struct EfRun {
    acx::EfLengths len;
    const int32_t *pairs;
    int64_t K;
    acx_ef_params p;
    acx::EfMode mode;
    int64_t batch_floats;
    bool rect_gemm;
};

// `ht`: ACX_EF_HOST_TIMING's seconds for descriptors [0] and rectangles [1]
static void prepare_ef_batch(acx_ctx *c, const EfRun &run, int64_t k_from, EfHostBatch &hb, double *ht)
{
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_a = now();
    hb.k_begin = k_from;
    hb.k_end = acx::ef_pack_batch(run.len, run.pairs, k_from, run.K, run.p, run.mode, run.batch_floats, hb.pd, hb.a);
    const double t_r = now();
    ht[0] += t_r - t_a;
    // the pairs of the batch laid out as dense rectangles (ef_gemm_rect_bf16x3_kernel)
    if (run.rect_gemm) ef_build_rects(hb.pd, c->h_efoff, c->ef_ntracks, hb.seg, hb.qslot, hb.rslot);
    ht[1] += now() - t_r;
}

// the one-row selection kernels (ACX_EF_ROW_2 / _4 / _LONG) in mode 0 (C), 1 (C^T) or 2 (the stored fused matrix)
static void launch_ef_rowstat(acx_ctx *c, int kernel, dim3 grid, int mode, int Kn)
{
    switch (kernel) {
    case ACX_EF_ROW_LONG:
        hipLaunchKernelGGL(acx::ef_rowstat_long_kernel, grid, dim3(256), 0, c->stream, c->d_efpd, c->d_scratch, c->d_thr, mode, Kn);
        break;
    case ACX_EF_ROW_4:
        hipLaunchKernelGGL((acx::ef_rowstat_kernel<4, false>), grid, dim3(256), 0, c->stream, c->d_efpd, c->d_scratch, c->d_thr, c->d_efbits, mode, Kn, 0);
        break;
    default:
        hipLaunchKernelGGL((acx::ef_rowstat_kernel<2, false>), grid, dim3(256), 0, c->stream, c->d_efpd, c->d_scratch, c->d_thr, c->d_efbits, mode, Kn, 0);
    }
}

// the fused matrix: made, thresholded and binarised row by row (stored too when keep_f)
template <int NQ>
static void launch_ef_fusesel(acx_ctx *c, dim3 grid, int Kn, int keep_f)
{
    if (c->ef_fuse == ACX_EF_FUSE_EXACT)
        hipLaunchKernelGGL((acx::ef_rowstat_kernel<NQ, true, true>), grid, dim3(256), 0, c->stream, c->d_efpd, c->d_scratch, c->d_thr, c->d_efbits, 3, Kn, keep_f);
    else
        hipLaunchKernelGGL((acx::ef_rowstat_kernel<NQ, true, false>), grid, dim3(256), 0, c->stream, c->d_efpd, c->d_scratch, c->d_thr, c->d_efbits, 3, Kn, keep_f);
}

// `src`: the matrix of the float kernels (0: every feature of the grid, 3: the fused one); the bit kernels walk every plane of the grid
static void launch_ef_sw(acx_ctx *c, int kernel, dim3 grid, int src)
{
    switch (kernel) {
    case ACX_EF_SW_H16_8:
        hipLaunchKernelGGL((acx::sw_bits_h16_kernel<8>), grid, dim3(64), 0, c->stream, c->d_efpd, c->d_efbits, c->d_out, 0);
        break;
    case ACX_EF_SW_H16_16:
        hipLaunchKernelGGL((acx::sw_bits_h16_kernel<16>), grid, dim3(64), 0, c->stream, c->d_efpd, c->d_efbits, c->d_out, 0);
        break;
    case ACX_EF_SW_8:
        hipLaunchKernelGGL((acx::sw_kernel<8>), grid, dim3(64), 0, c->stream, c->d_efpd, c->d_scratch, c->d_thr, c->d_out, src);
        break;
    case ACX_EF_SW_16:
        hipLaunchKernelGGL((acx::sw_kernel<16>), grid, dim3(64), 0, c->stream, c->d_efpd, c->d_scratch, c->d_thr, c->d_out, src);
        break;
    default:
        hipLaunchKernelGGL(acx::sw_long_kernel, grid, dim3(64), 0, c->stream, c->d_efpd, c->d_scratch, c->d_thr, c->d_out, src);
    }
}

// A batch on the device: its arenas and descriptors, then every launch of it, the kernels as the plan names them (`kn`:
// ef_batch_kernels, ef_plan.hpp).  ext_matrix (test entries): the caller's extM x extN matrix is "feature 0" of the one pair.
static int launch_ef_batch(acx_ctx *c, const EfHostBatch &hb, const acx::EfBatchKernels &kn, const acx::EfMode &mode, const acx_ef_params &p,
                           const float *ext_matrix, int extM, int extN)
{
    const int B = (int)hb.pd.size(), maxM = hb.a.maxM, maxN = hb.a.maxN;
    const int64_t cells = hb.a.cells;
    int rc;
    if ((rc = ensure(c, c->d_scratch, (size_t)hb.a.used)) != ACX_OK) return rc;
    if ((rc = ensure(c, c->d_thr, (size_t)hb.a.used_s)) != ACX_OK) return rc;
    if ((rc = ensure(c, c->d_efbits, (size_t)hb.a.used_b)) != ACX_OK) return rc;
    if ((rc = ensure(c, c->d_efpd, (size_t)B)) != ACX_OK) return rc;
    if ((rc = ensure(c, c->d_out, (size_t)4 * B)) != ACX_OK) return rc;
    ACX_HIP(c, hipMemcpyAsync(c->d_efpd, hb.pd.data(), sizeof(acx::EfPair) * B, hipMemcpyHostToDevice, c->stream));
    if (ext_matrix) {
        ACX_HIP(c, hipMemcpy2DAsync(c->d_scratch, sizeof(float) * hb.pd[0].pitchC, ext_matrix, sizeof(float) * extN,
                                    sizeof(float) * extN, extM, hipMemcpyHostToDevice, c->stream));
    } else {
        hipLaunchKernelGGL(acx::ef_oti_kernel, dim3((B + 255) / 256), dim3(256), 0, c->stream, c->d_efpd, B, c->d_efmed);
        const int tiles_x = (maxN + acx::EF_TILE - 1) / acx::EF_TILE, tiles_y = (maxM + acx::EF_TILE - 1) / acx::EF_TILE;
        ProfScope ps(c, KS_EFGEMM, cells);
        if ((rc = launch_ef_gemms(c, hb.seg, B, tiles_x, tiles_y)) != ACX_OK) return rc;
    }
    const int nfeat = ext_matrix ? 1 : 3;
    const int rows_g = (std::max(maxM, maxN) + 3) / 4;
    {
        ProfScope ps(c, KS_EFSTAT, cells);
        if (kn.row == ACX_EF_ROW_TWO)
            hipLaunchKernelGGL(acx::ef_rowstat2_kernel, dim3((maxM + 7) / 8, B, nfeat), dim3(256), 0, c->stream, c->d_efpd, c->d_scratch, c->d_thr,
                               c->d_efbits, p.K);
        else
            launch_ef_rowstat(c, kn.row, dim3(rows_g, B, nfeat), 0, p.K);
        switch (kn.col) {
        case ACX_EF_COL_ROWPASS:
            launch_ef_rowstat(c, kn.row1, dim3(rows_g, B, 3), 1, p.K);
            break;
        case ACX_EF_COL_10:
            hipLaunchKernelGGL((acx::ef_colstat_kernel<10>), dim3((maxN + 63) / 64, B, 3), dim3(256), 0, c->stream, c->d_efpd, c->d_scratch, c->d_thr, p.K);
            break;
        case ACX_EF_COL_16:
            hipLaunchKernelGGL((acx::ef_colstat_kernel<acx::EF_COLSTAT_MAXK>), dim3((maxN + 63) / 64, B, 3), dim3(256), 0, c->stream, c->d_efpd, c->d_scratch, c->d_thr, p.K);
            break;
        default:          // (a caller's matrix: threshold = kbin smallest per row, no columns)
            break;
        }
    }
    if (mode.bits_path) {
        if (kn.fuse != ACX_EF_FUSE_NONE) {
            ProfScope ps(c, KS_EFFUSE, cells);
            if (kn.fuse == ACX_EF_FUSE_WIDE) launch_ef_fusesel<4>(c, dim3((maxM + 3) / 4, B, 1), p.K, mode.keep_f ? 1 : 0);
            else launch_ef_fusesel<2>(c, dim3((maxM + 3) / 4, B, 1), p.K, mode.keep_f ? 1 : 0);
        }
        ProfScope ps(c, KS_EFSW, cells);
        launch_ef_sw(c, kn.sw, dim3(B, ext_matrix ? 1 : 4), 0);
    } else {
        {
            ProfScope ps(c, KS_EFSW, cells);
            launch_ef_sw(c, kn.sw, dim3(B, nfeat), 0);
        }
        if (kn.fuse == ACX_EF_FUSE_FLOAT) {
            {
                ProfScope ps(c, KS_EFFUSE, cells);
                hipLaunchKernelGGL(acx::ef_fuse_kernel, dim3(maxM, B), dim3(256), 0, c->stream, c->d_efpd, c->d_scratch, c->d_thr, c->ef_fuse == ACX_EF_FUSE_EXACT ? 1 : 0);
            }
            {
                ProfScope ps(c, KS_EFSTAT, 0);
                launch_ef_rowstat(c, kn.row1, dim3(rows_g, B, 1), 2, p.K);
            }
            {
                ProfScope ps(c, KS_EFSW, 0);
                launch_ef_sw(c, kn.sw, dim3(B, 1), 3);
            }
        }
    }
    ACX_LAUNCHES_OK(c);
    return ACX_OK;
}

// The four scores of the batch's pairs, queued behind its kernels: to out[4 k ..] on the host, or (`dd`, grid runs) to
// dd->base[dd->idx[k] .. + 4) on the DEVICE.
static int copy_ef_scores(acx_ctx *c, const EfHostBatch &hb, float *out, const DevDst *dd)
{
    const int B = (int)hb.pd.size();
    if (!dd) {
        ACX_HIP(c, hipMemcpyAsync(out + 4 * hb.k_begin, c->d_out, sizeof(float) * 4 * B, hipMemcpyDeviceToHost, c->stream));
        return ACX_OK;
    }
    const int rc = stage_idx(c, dd->idx + hb.k_begin, B);
    if (rc != ACX_OK) return rc;
    hipLaunchKernelGGL(scatter_scores_kernel, dim3((B + 255) / 256), dim3(256), 0, c->stream, c->d_out, c->d_idx, dd->base, B, 4);
    ACX_HIP(c, hipGetLastError());
    return ACX_OK;
}

// The debug entries: what the (one) batch left behind for its pair `which`, on an idle stream.  `ext`: a caller's matrix has one
// slot and no column means; a pair of the pool three features and the fused slot.
static int ef_debug_readback(acx_ctx *c, const EfDebug &dbg, int64_t which, bool ext)
{
    acx::EfPair d;
    ACX_HIP(c, hipMemcpy(&d, c->d_efpd + which, sizeof(acx::EfPair), hipMemcpyDeviceToHost));
    if (dbg.oti) *dbg.oti = d.oti;
    for (int sft = 0; sft < 3 && dbg.csm; ++sft)
        ACX_HIP(c, hipMemcpy2D(dbg.csm + (size_t)sft * d.M * d.N, sizeof(float) * d.N,
                               c->d_scratch + d.offC + (int64_t)sft * d.M * d.pitchC, sizeof(float) * d.pitchC,
                               sizeof(float) * d.N, d.M, hipMemcpyDeviceToHost));
    if (dbg.fused)
        ACX_HIP(c, hipMemcpy2D(dbg.fused, sizeof(float) * d.N,
                               c->d_scratch + d.offC + (int64_t)3 * d.M * d.pitchC + (int64_t)3 * d.ctN * d.pitchT,
                               sizeof(float) * d.pitchC, sizeof(float) * d.N, d.M, hipMemcpyDeviceToHost));
    const EfStats *st = dbg.stats;
    if (!st) return ACX_OK;
    // the vectors of d_thr (layout: ef_kernels.hpp, EfPair::offS) and the words of d_efbits as the kernels wrote them
    const int nf = ext ? 1 : 3, nslots = ext ? 1 : 4;
    const int64_t stride = acx::ef_s_stride(d);
    if (st->bits)
        ACX_HIP(c, hipMemcpy(st->bits, c->d_efbits + d.offB, sizeof(uint32_t) * (size_t)nslots * d.M * (d.pitchC / 32), hipMemcpyDeviceToHost));
    for (int sl = 0; sl < nslots; ++sl) {
        const float *S = c->d_thr + d.offS + sl * stride;
        if (st->t) ACX_HIP(c, hipMemcpy(st->t + (size_t)sl * d.M, S, sizeof(float) * d.M, hipMemcpyDeviceToHost));
        if (st->jcut) ACX_HIP(c, hipMemcpy(st->jcut + (size_t)sl * d.M, S + acx::ef_jcut_off(d, sl), sizeof(int32_t) * d.M, hipMemcpyDeviceToHost));
        if (sl >= nf) continue;
        if (st->r) ACX_HIP(c, hipMemcpy(st->r + (size_t)sl * d.M, S + d.pitchT, sizeof(float) * d.M, hipMemcpyDeviceToHost));
        if (st->c && !ext) ACX_HIP(c, hipMemcpy(st->c + (size_t)sl * d.N, S + 2 * d.pitchT, sizeof(float) * d.N, hipMemcpyDeviceToHost));
    }
    return ACX_OK;
}

// The scratch limit of a run in floats: the context's, else ACX_SCRATCH_GB, else 36 GB (a whole 128 x 128 grid tile of 400-block
// tracks -- 16 384 pairs, three float matrices each since the transposed and the fused matrices are gone -- in one batch).  Much
// larger batches buy nothing (measured with the 7-matrix layout: 98 k pairs/s at 24 GB, 101 k at 115 GB, 94 k at 8 GB) and the
// first hipMalloc of a 100 GB arena costs 3.4 s
static int64_t ef_scratch_limit(const acx_ctx *c)
{
    if (c->scratch_limit > 0) return c->scratch_limit;
    const char *env = getenv("ACX_SCRATCH_GB");
    if (env && atof(env) > 0) return (int64_t)(atof(env) * (double)(1ull << 30));
    return std::min<int64_t>((int64_t)(0.40 * (double)c->total_mem), (int64_t)36 << 30);
}

// The pool is up and the WHOLE list is good (ef_check_pairs, ef_plan.hpp), before the first launch: a bad pair behind the first
// batch fails the call before any batch has run, as the reference fails a chunk (algorithm_template.py:174-177).  No pool: that,
// whatever the indices are.  `upto` (or nullptr): the pair the list is good up to, where a caller's own per-pair rules come
// before a track without blocks -- then ACX_ERR_SHORT is the caller's to report (ef_short_pair) once its rules have passed them.
static int ef_short_pair(acx_ctx *c, int64_t k) { return fail(c, ACX_ERR_SHORT, "earlyfusion: track without blocks (pair " + std::to_string(k) + ")"); }

// (the texts of ef_check_pairs' answers; c == nullptr: for acx_last_error(NULL))
static int ef_check_text(acx_ctx *c, const acx::EfCheck &ck)
{
    if (ck.code == ACX_ERR_INVALID) return fail(c, ACX_ERR_INVALID, "earlyfusion: track index out of range in pair " + std::to_string(ck.k));
    return ck.code == ACX_ERR_SHORT ? ef_short_pair(c, ck.k) : ACX_OK;
}

static int check_ef_pairs(acx_ctx *c, const int32_t *pairs, int64_t K, int64_t *upto = nullptr)
{
    if (!c->d_ef[0] || c->ef_open) return fail(c, ACX_ERR_STATE, "earlyfusion: block-feature pool not uploaded (acx_ef_upload_pool)");
    const acx::EfCheck ck = acx::ef_check_pairs(acx::EfLengths{c->h_efoff.data(), c->ef_ntracks}, pairs, K);
    if (upto && ck.code != ACX_ERR_INVALID) { *upto = ck.k; return ACX_OK; }
    return ef_check_text(c, ck);
}

// `dd` (grid runs): the four scores of pair k go to dd->base[dd->idx[k] .. + 4) on the DEVICE instead of out[4 k ..].  `pd_out`
// (the cross-diffusion fusion): the caller goes on with the matrices this call leaves in d_scratch, where the descriptors of its
// ONE batch say.  (Behind run_ef's guard, below.)
static int run_ef_impl(acx_ctx *c, const int32_t *pairs, int64_t K, const acx_ef_params &p, float *out, const EfDebug *dbg,
                       const float *ext_matrix, int extM, int extN, const DevDst *dd, const EfAlign *aln, std::vector<acx::EfPair> *pd_out)
{
    int rc;
    if (!ext_matrix && (!c->d_ef[0] || c->ef_open)) return fail(c, ACX_ERR_STATE, "earlyfusion: block-feature pool not uploaded (acx_ef_upload_pool)");
    if (!(p.kappa >= 0.0)) return fail(c, ACX_ERR_INVALID, "earlyfusion: kappa must be >= 0");
    if (p.K < 1) return fail(c, ACX_ERR_INVALID, "earlyfusion: K must be >= 1");
    ACX_HIP(c, hipSetDevice(c->device));
    if (!ext_matrix && (rc = check_ef_pairs(c, pairs, K)) != ACX_OK) return rc;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_call = now();
    const int64_t limit = ef_scratch_limit(c), limit_floats = limit / 4;
    const bool want_fused = dbg && dbg->fused;
    const acx::EfLengths len{c->h_efoff.data(), c->ef_ntracks};
    const acx::EfMode mode = ext_matrix ? acx::ef_mode_matrix(extM, extN, want_fused) : acx::ef_mode(len, pairs, K, p.K, want_fused);
    EfRun run{len, pairs, K, p, mode, limit_floats, !ext_matrix && c->ef_gemm != ACX_EF_GEMM_F32 && c->ef_gemm != ACX_EF_GEMM_BF16X3_PAIRWISE};
    if (aln && (ext_matrix || dd || !out))          // (no export gets here: acx_ef_align passes the pool's pairs and a host buffer)
        return fail(c, ACX_ERR_STATE, "ef_align: the alignment option takes pairs of the pool and scores on the host");
    if (aln && !mode.bits_path && !aln->any_length)
        return fail(c, ACX_ERR_UNSUPPORTED, "ef_align: alignment needs the bit path: at most 1024 blocks");
    if (dbg && dbg->stats && dbg->stats->bits && !mode.bits_path)
        return fail(c, ACX_ERR_INVALID, "ef debug: a track of more than 1024 blocks takes the float path, which leaves no bitmaps (pass a null bitmap pointer)");
    // development aid (ACX_EF_HOST_TIMING=1): where the HOST's time of a call goes -- descriptors, rectangles, enqueue, waiting for the device
    static const bool host_timing = [] { const char *e = getenv("ACX_EF_HOST_TIMING"); return e && e[0] == '1'; }();
    double ht[5] = {0, 0, 0, 0, 0};
    int nbatches = 0;
    EfHostBatch hbs[2];
    if (ext_matrix) {
        // test entries: the caller's matrix as the one pair of the one batch
        EfHostBatch &hb = hbs[0];
        hb.pd.assign(1, acx::ef_pair_desc(0, 0, extM, extN, p.kappa, false));
        if (acx::ef_pair_floats(hb.pd[0], mode.keep_f) > limit_floats) return fail(c, ACX_ERR_NOMEM, "earlyfusion: one pair does not fit the scratch limit");
        acx::ef_arena_add(hb.a, hb.pd[0], mode.keep_f);
        hb.k_end = K;
        ht[4] = now() - t_call;
    } else {
        // (the last of the up-front checks: a pair that cannot fit the scratch limit on its own)
        const acx::EfSizes sz = acx::ef_batch_floats(run.len, pairs, K, p.kappa, mode, limit_floats);
        if (sz.too_big >= 0) return fail(c, ACX_ERR_NOMEM, "earlyfusion: pair " + std::to_string(sz.too_big) + " does not fit the scratch limit");
        run.batch_floats = sz.batch_floats;
        ht[4] = now() - t_call;
        prepare_ef_batch(c, run, 0, hbs[0], ht);
        if (dbg && hbs[0].k_end < K)          // the debug entries show one batch: refused before the first launch
            return fail(c, ACX_ERR_UNSUPPORTED, "ef debug: the list does not fit one batch");
        if (pd_out && hbs[0].k_end < K) return fail(c, ACX_ERR_NOMEM, "earlyfusion: the pair and its two self pairs do not fit the scratch limit");
    }
    for (int bi = 0; hbs[bi & 1].k_begin < K; ++bi) {
        EfHostBatch &hb = hbs[bi & 1];
        ++nbatches;
        const double t_b = now();
        const acx::EfBatchKernels kn = acx::ef_batch_kernels(hb.a.maxM, hb.a.maxN, p.K, mode, ext_matrix != nullptr);
        if ((rc = launch_ef_batch(c, hb, kn, mode, p, ext_matrix, extM, extN)) != ACX_OK) return rc;
        if ((rc = copy_ef_scores(c, hb, out, dd)) != ACX_OK) return rc;
        // acx_ef_align / acx_ef_align_long: the records (and paths) of this batch, while d_efbits (the float path: d_scratch and d_thr)
        // still holds it
        if (aln && (rc = run_ef_align_batch(c, hb.pd, hb.k_begin, limit / 2, *aln, out + 4 * hb.k_begin, !mode.bits_path)) != ACX_OK) return rc;
        const double t_s = now();
        ht[2] += t_s - t_b;
        // the next batch's descriptors and rectangles, while the device works on this one
        EfHostBatch &nx = hbs[(bi & 1) ^ 1];
        nx.k_begin = K;
        if (hb.k_end < K) prepare_ef_batch(c, run, hb.k_end, nx, ht);
        const double t_w = now();
        ACX_HIP(c, hipStreamSynchronize(c->stream));
        ht[3] += now() - t_w;
        drain_profile(c);
        if (pd_out) *pd_out = hb.pd;
        if (dbg && (rc = ef_debug_readback(c, *dbg, dbg->which - hb.k_begin, ext_matrix != nullptr)) != ACX_OK) return rc;
    }
    if (host_timing)
        fprintf(stderr, "[acx ef host] %lld pairs in %d batches, %.1f ms: preamble %.1f, descriptors %.1f, rectangles %.1f, enqueue %.1f, waiting for the device %.1f\n",
                (long long)K, nbatches, 1e3 * (now() - t_call), 1e3 * ht[4], 1e3 * ht[0], 1e3 * ht[1], 1e3 * ht[2], 1e3 * ht[3]);
    return ACX_OK;
}

int run_ef(acx_ctx *c, const int32_t *pairs, int64_t K, const acx_ef_params &p, float *out, const EfDebug *dbg,
           const float *ext_matrix, int extM, int extN, const DevDst *dd = nullptr, const EfAlign *aln = nullptr,
           std::vector<acx::EfPair> *pd_out = nullptr)
{
    return guarded(c, [&] { return run_ef_impl(c, pairs, K, p, out, dbg, ext_matrix, extM, extN, dd, aln, pd_out); });
}

static void free_pool(acx_ctx *c)
{
    for (DeviceBuffer<float> *b : {&c->d_frames0, &c->d_frames, &c->d_frot, &c->d_normtab, &c->d_gch}) (void)b->reset();
    for (DeviceBuffer<int64_t> *b : {&c->d_toff0, &c->d_toff, &c->d_noff}) (void)b->reset();
    (void)c->d_fh.reset();
    (void)c->d_planes.reset();
    c->normtab_m = 0; c->normtab_span = -1;
    c->pool_tau = 0;
    c->fh_base_n = -1;
}

template <int L>
int launch_simple(acx_ctx *c, int n, size_t smem, int oti)
{
    auto kern = acx::simple_kernel<L>;
    // waves (= pairs) per workgroup: SIMPLE_WPB, fewer when the tracks are long enough for their LDS to run out
    int wpb = acx::SIMPLE_WPB;
    while (wpb > 1 && smem * wpb > 160 * 1024) --wpb;
    ACX_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(smem * wpb)));
    hipLaunchKernelGGL(kern, dim3((n + wpb - 1) / wpb), dim3(64 * wpb), smem * wpb, c->stream, c->d_frames64, c->d_toff64,
                       c->d_prof64, c->d_wn64, c->d_pairs, c->d_out64, oti, n, (int)smem);
    return ACX_OK;
}

// simple_kernel's LDS per wave for tracks of up to maxn frames: the hand-over row + the profile keys
static size_t simple_smem(int maxn) { return 64 + sizeof(double) * (2 * (size_t)maxn + (size_t)maxn / 48 + 4); }

static int launch_simple_sslen(acx_ctx *c, int sslen, int n, size_t smem, int oti)
{
    switch (sslen) {
#define ACX_L(L_) case L_: return launch_simple<L_>(c, n, smem, oti);
        ACX_L(1) ACX_L(2) ACX_L(3) ACX_L(4) ACX_L(5) ACX_L(6) ACX_L(7) ACX_L(8)
        ACX_L(9) ACX_L(10) ACX_L(11) ACX_L(12) ACX_L(13) ACX_L(14) ACX_L(15) ACX_L(16)
#undef ACX_L
    }
    return fail(c, ACX_ERR_UNSUPPORTED, "simple: SSLEN must be in 1..16 on the device");
}

// simple_profile_kernel's LDS per wave: simple_kernel's + the profile's index (4 bytes per row, kept a multiple of 16)
static size_t simple_profile_smem(int maxn) { return simple_smem(maxn) + (4 * (size_t)maxn + 15) / 16 * 16; }

// d_poff: where each pair's profile starts in d_mp / d_mpi; nullptr: the records alone
template <int L>
int launch_simple_profile(acx_ctx *c, int n, size_t smem, int oti, const int64_t *d_poff)
{
    auto kern = acx::simple_profile_kernel<L>;
    int wpb = acx::SIMPLE_WPB;                        // the step-down of launch_simple
    while (wpb > 1 && smem * wpb > 160 * 1024) --wpb;
    ACX_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(smem * wpb)));
    hipLaunchKernelGGL(kern, dim3((n + wpb - 1) / wpb), dim3(64 * wpb), smem * wpb, c->stream, c->d_frames64, c->d_toff64,
                       c->d_prof64, c->d_wn64, c->d_pairs, c->d_sprec, d_poff, c->d_spmp, c->d_spmpi, oti, n, (int)smem);
    return ACX_OK;
}

static int launch_simple_profile_sslen(acx_ctx *c, int sslen, int n, size_t smem, int oti, const int64_t *d_poff)
{
    switch (sslen) {
#define ACX_L(L_) case L_: return launch_simple_profile<L_>(c, n, smem, oti, d_poff);
        ACX_L(1) ACX_L(2) ACX_L(3) ACX_L(4) ACX_L(5) ACX_L(6) ACX_L(7) ACX_L(8)
        ACX_L(9) ACX_L(10) ACX_L(11) ACX_L(12) ACX_L(13) ACX_L(14) ACX_L(15) ACX_L(16)
#undef ACX_L
    }
    return fail(c, ACX_ERR_UNSUPPORTED, "simple_profile: SSLEN must be in 1..16 on the device");
}

// |x_t|^2 summed over every window of `sslen` frames of the f64 pool: built on first use per (pool, SSLEN)
static int ensure_winnorm(acx_ctx *c, int sslen)
{
    if (c->d_wn64 && c->wn64_L == sslen) return ACX_OK;
    ACX_HIP(c, c->d_wn64.reset());
    c->wn64_L = 0;
    const int64_t total = c->h_off64[c->n_tracks64];
    int maxn = 1;
    for (int t = 0; t < c->n_tracks64; ++t) maxn = std::max<int>(maxn, (int)(c->h_off64[t + 1] - c->h_off64[t]));
    ACX_HIP(c, c->d_wn64.grow((size_t)std::max<int64_t>(1, total)));
    ACX_HIP(c, hipMemsetAsync(c->d_wn64, 0, sizeof(double) * std::max<int64_t>(1, total), c->stream));
    // (grid.x = tracks: up to 2^31 - 1)
    hipLaunchKernelGGL(acx::simple_winnorm_kernel, dim3(c->n_tracks64, std::min(64, (maxn + 255) / 256)), dim3(256), 0, c->stream,
                       c->d_frames64, c->d_toff64, c->d_wn64, sslen);
    ACX_HIP(c, hipGetLastError());
    c->wn64_L = sslen;
    return ACX_OK;
}

// What the device-resident SiMPle runs do before their first launch: SSLEN and the length of every track that
// each_track(visit) visits are checked, *smem is set for the longest of them and the window norms are there.
template <typename Each>
static int simple_front(acx_ctx *c, int sslen, Each each_track, size_t *smem)
{
    if (sslen < 1 || sslen > acx::SIMPLE_MAXL) return fail(c, ACX_ERR_UNSUPPORTED, "simple: SSLEN must be in 1..16 on the device");
    int maxn = 0, rc = ACX_OK;
    each_track([&](int t) {
        const int n = (int)(c->h_off64[t + 1] - c->h_off64[t]);
        if (rc != ACX_OK) return;                     // (the first finding stands)
        if (n < sslen) rc = fail(c, ACX_ERR_SHORT, "simple: track " + std::to_string(t) + " is shorter than SSLEN");
        else if (n > acx::SIMPLE_MAXN) rc = fail(c, ACX_ERR_UNSUPPORTED, "simple: tracks with more than 6000 pooled frames are not supported on the device");
        maxn = std::max(maxn, n);
    });
    if (rc != ACX_OK) return rc;
    *smem = simple_smem(maxn);
    return ensure_winnorm(c, sslen);
}

// The tile descriptors of a launch in c->d_tiles (grown as needed; pageable source: the copy is staged before the call
// returns, the host's copy may be reused at once)
static int upload_tiles(acx_ctx *c, const void *tiles, size_t bytes)
{
    if (const int rc = ensure(c, c->d_tiles, bytes); rc != ACX_OK) return rc;
    ACX_HIP(c, hipMemcpyAsync(c->d_tiles, tiles, bytes, hipMemcpyHostToDevice, c->stream));
    return ACX_OK;
}

// ---------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------
extern "C" {

int acx_abi_version(void) { return ACX_ABI_VERSION; }

int acx_hip_versions(int *build, int *runtime)
{
    if (build) *build = HIP_VERSION;
    int v = 0;
    if (runtime) *runtime = hipRuntimeGetVersion(&v) == hipSuccess ? v : 0;
    return 0;
}

acx_ctx *acx_create(int device, int *err)
{
    auto bad = [&](int code, const std::string &msg) -> acx_ctx * {
        g_create_error = msg;
        if (err) *err = code;
        return nullptr;
    };
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return bad(ACX_ERR_HIP, std::string("no HIP device: ") + hipGetErrorString(e));
    if (device < 0 || device >= n) return bad(ACX_ERR_INVALID, "device index out of range");
    if ((e = hipSetDevice(device)) != hipSuccess) return bad(ACX_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return bad(ACX_ERR_HIP, std::string("hipGetDeviceProperties: ") + hipGetErrorString(e));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return bad(ACX_ERR_HIP, std::string("libacx is built for gfx950 only; device is ") + prop.gcnArchName);
    acx_ctx *c = new acx_ctx();
    c->device = device;
    c->total_mem = prop.totalGlobalMem;
    c->n_cu = prop.multiProcessorCount;
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) {
        delete c;
        return bad(ACX_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    if (err) *err = ACX_OK;
    return c;
}

static void comm_release(acx_ctx *c);

void acx_destroy(acx_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->qstream) (void)hipStreamSynchronize(c->qstream);
    if (c->qstream2) (void)hipStreamSynchronize(c->qstream2);
    comm_release(c);
    drain_profile(c);
    for (hipEvent_t ev : c->event_pool) (void)hipEventDestroy(ev);
    for (Serra09Slot &sl : c->slot) {
        if (sl.done) (void)hipEventDestroy(sl.done);
        for (hipEvent_t ev : sl.cls_ev)
            if (ev) (void)hipEventDestroy(ev);
    }
    for (hipEvent_t ev : c->rank_ev)
        if (ev) (void)hipEventDestroy(ev);
    if (c->q2_done) (void)hipEventDestroy(c->q2_done);
    if (c->qstream) (void)hipStreamDestroy(c->qstream);
    if (c->qstream2) (void)hipStreamDestroy(c->qstream2);
    (void)hipStreamDestroy(c->stream);
    delete c;                                    // (every device and pinned buffer frees itself with the context)
}

#ifdef ACX_EF_TIMING
extern "C" int acx_ef_clk(unsigned long long *out, int reset)
{
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(acx::g_ef_clk), sizeof(unsigned long long) * 16) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[16] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(acx::g_ef_clk), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif

const char *acx_last_error(const acx_ctx *c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int acx_set_scratch_limit(acx_ctx *c, int64_t bytes)
{
    if (!c) return ACX_ERR_INVALID;
    c->scratch_limit = bytes < 0 ? 0 : bytes;
    return ACX_OK;
}

int acx_set_nonfinite_policy(acx_ctx *c, int32_t policy)
{
    if (!c) return ACX_ERR_INVALID;
    if (policy != ACX_NONFINITE_REJECT && policy != ACX_NONFINITE_ZERO) return fail(c, ACX_ERR_INVALID, "set_nonfinite_policy: unknown policy");
    c->nonfinite_policy = policy;
    return ACX_OK;
}

int64_t acx_nonfinite_zeroed(const acx_ctx *c) { return c ? c->nf_zeroed : 0; }

static int upload_pool_impl(acx_ctx *c, const float *frames, const int64_t *offsets, int32_t n_tracks, int32_t dim);
static int fill_pool(acx_ctx *c, const float *frames, const int64_t *offsets, int32_t n_tracks, int32_t dim);
static int upload_pool_f64_impl(acx_ctx *c, const double *frames, const int64_t *offsets, int32_t n_tracks, int32_t dim);

int acx_upload_pool(acx_ctx *c, const float *frames, const int64_t *offsets, int32_t n_tracks, int32_t dim)
{
    if (!c) return ACX_ERR_INVALID;
    c->nf_zeroed = 0;
    return upload_pool_impl(c, frames, offsets, n_tracks, dim);
}

static int upload_pool_impl(acx_ctx *c, const float *frames, const int64_t *offsets, int32_t n_tracks, int32_t dim)
{
    if (!frames || !offsets || n_tracks <= 0 || dim <= 0) return fail(c, ACX_ERR_INVALID, "upload_pool: bad argument");
    if (offsets[0] != 0) return fail(c, ACX_ERR_INVALID, "upload_pool: offsets[0] must be 0");
    for (int i = 0; i < n_tracks; ++i)
        if (offsets[i + 1] < offsets[i]) return fail(c, ACX_ERR_INVALID, "upload_pool: offsets must be non-decreasing");
    ACX_HIP(c, hipSetDevice(c->device));
    free_pool(c);
    const int rc = fill_pool(c, frames, offsets, n_tracks, dim);
    if (rc != ACX_OK) { free_pool(c); c->n_tracks = 0; }      // whatever failed: no pool, the next call says so (ACX_ERR_STATE)
    return rc;
}

static int fill_pool(acx_ctx *c, const float *frames, const int64_t *offsets, int32_t n_tracks, int32_t dim)
{
    const int64_t total = offsets[n_tracks];
    c->h_off0.assign(offsets, offsets + n_tracks + 1);
    c->n_tracks = n_tracks;
    c->dim = dim;
    ACX_HIP(c, c->d_frames0.grow((size_t)std::max<int64_t>(1, total) * dim));
    ACX_HIP(c, c->d_toff0.grow((size_t)n_tracks + 1));
    ACX_HIP(c, hipMemcpy(c->d_frames0, frames, sizeof(float) * total * dim, hipMemcpyHostToDevice));
    ACX_HIP(c, hipMemcpy(c->d_toff0, offsets, sizeof(int64_t) * (n_tracks + 1), hipMemcpyHostToDevice));
    {
        const int rc = scan_nonfinite(c, "upload_pool", "frames", c->d_frames0.get(), total * dim, dim, 0, c->d_toff0.get(), n_tracks);
        if (rc != ACX_OK) return rc;
    }
    std::vector<float> cleaned;                     // policy ZERO and something was zeroed: the host-side sums below see what the device holds
    if (c->nf_zeroed > 0 && dim == acx::NBIN) {
        cleaned.resize((size_t)total * dim);
        ACX_HIP(c, hipMemcpy(cleaned.data(), c->d_frames0, sizeof(float) * total * dim, hipMemcpyDeviceToHost));
        frames = cleaned.data();
    }
    if (dim == acx::NBIN) {
        // the active pool (rotated copy included) for the default stack stride
        const int rc = ensure_tau(c, 1);
        if (rc != ACX_OK) return rc;
        // global chroma profile per track: sequential f32 sum over frames, divided by its max
        // (arithmetic spec step 1; O(sum T) host work done once per pool)
        std::vector<float> g((size_t)n_tracks * acx::NBIN);
        for (int t = 0; t < n_tracks; ++t) {
            float acc[acx::NBIN];
            for (int b = 0; b < acx::NBIN; ++b) acc[b] = 0.0f;
            const float *x = frames + offsets[t] * dim;
            const int64_t T = offsets[t + 1] - offsets[t];
            for (int64_t f = 0; f < T; ++f)
                for (int b = 0; b < acx::NBIN; ++b) acc[b] = acc[b] + x[f * acx::NBIN + b];
            float mx = acc[0];
            for (int b = 1; b < acx::NBIN; ++b) if (acc[b] > mx) mx = acc[b];
            for (int b = 0; b < acx::NBIN; ++b) g[(size_t)t * acx::NBIN + b] = (mx > 0.0f) ? acc[b] / mx : acc[b];
        }
        ACX_HIP(c, c->d_gch.grow(g.size()));
        ACX_HIP(c, hipMemcpy(c->d_gch, g.data(), sizeof(float) * g.size(), hipMemcpyHostToDevice));
    }
    return ACX_OK;
}

// Raw pools are prepared in slices of whole tracks (for_track_slices) so that the staging buffer stays bounded
// whatever the collection size (a 15 k-track collection is ~60 GB of raw chroma): 1 GiB of raw features, or the
// scratch limit where acx_set_scratch_limit set a smaller one.  Every preparation kernel works per track, so
// where the slices end changes no result.
static const int64_t RAW_SLICE_FLOATS = (int64_t)1 << 28;       // 1 GiB of f32

static int64_t raw_slice_bytes(const acx_ctx *c)
{
    const int64_t bytes = RAW_SLICE_FLOATS * (int64_t)sizeof(float);
    return c->scratch_limit > 0 ? std::min(bytes, c->scratch_limit) : bytes;
}

static int check_raw_args(acx_ctx *c, const char *who, const float *raw, const int64_t *roff, int32_t n_tracks, int32_t dim)
{
    if (!raw || !roff || n_tracks <= 0 || dim != 12) return fail(c, ACX_ERR_INVALID, std::string(who) + ": bad argument (dim must be 12)");
    if (roff[0] != 0) return fail(c, ACX_ERR_INVALID, std::string(who) + ": offsets[0] must be 0");
    for (int i = 0; i < n_tracks; ++i)
        if (roff[i + 1] < roff[i]) return fail(c, ACX_ERR_INVALID, std::string(who) + ": offsets must be non-decreasing");
    return ACX_OK;
}

int acx_upload_raw_pool(acx_ctx *c, const float *raw, const int64_t *raw_offsets, int32_t n_tracks, int32_t dim,
                        int32_t fac, int64_t *pooled_offsets_out)
{
    if (!c) return ACX_ERR_INVALID;
    int rc;
    if ((rc = check_raw_args(c, "upload_raw_pool", raw, raw_offsets, n_tracks, dim)) != ACX_OK) return rc;
    if (fac < 1) return fail(c, ACX_ERR_INVALID, "upload_raw_pool: downsample factor must be >= 1");
    if (fac > acx::POOL_MAXFAC) return fail(c, ACX_ERR_UNSUPPORTED, "upload_raw_pool: downsample factors above 64 are not supported on the device");
    ACX_HIP(c, hipSetDevice(c->device));
    c->nf_zeroed = 0;
    std::vector<int64_t> poff((size_t)n_tracks + 1, 0);
    for (int t = 0; t < n_tracks; ++t) {
        const int64_t T0 = raw_offsets[t + 1] - raw_offsets[t];
        poff[t + 1] = poff[t] + (T0 + fac - 1) / fac;            // boundaries unique({0, fac, 2 fac, ..., T0})
    }
    const int64_t ptotal = poff[n_tracks];
    std::vector<float> pooled((size_t)std::max<int64_t>(1, ptotal) * 12);
    DeviceBuffer<int64_t> d_roff, d_poff;
    DeviceBuffer<float> d_raw, d_pooled;             // staging of one slice: grown as needed, reused by the next
    ACX_HIP(c, d_roff.grow((size_t)n_tracks + 1));
    ACX_HIP(c, d_poff.grow((size_t)n_tracks + 1));
    ACX_HIP(c, hipMemcpy(d_roff, raw_offsets, sizeof(int64_t) * (n_tracks + 1), hipMemcpyHostToDevice));
    ACX_HIP(c, hipMemcpy(d_poff, poff.data(), sizeof(int64_t) * (n_tracks + 1), hipMemcpyHostToDevice));
    const int64_t budget = raw_slice_bytes(c);
    rc = for_track_slices(
        n_tracks, n_tracks, [&](int t0, int t1) { return (raw_offsets[t1] - raw_offsets[t0]) * 12 * (int64_t)sizeof(float) <= budget; },
        [&](int t0, int t1) -> int {
            const int64_t nraw = raw_offsets[t1] - raw_offsets[t0], npool = poff[t1] - poff[t0];
            if (npool <= 0) return ACX_OK;
            ACX_HIP(c, d_raw.grow((size_t)nraw * 12));
            ACX_HIP(c, d_pooled.grow((size_t)npool * 12));
            ACX_HIP(c, hipMemcpyAsync(d_raw, raw + raw_offsets[t0] * 12, sizeof(float) * nraw * 12, hipMemcpyHostToDevice, c->stream));
            const int rcs = scan_nonfinite(c, "upload_raw_pool", "raw chroma", d_raw.get(), nraw * 12, 12, raw_offsets[t0], d_roff.get(), n_tracks);
            if (rcs != ACX_OK) return rcs;
            const int64_t blocks = (npool + acx::POOL_FPB - 1) / acx::POOL_FPB;
            hipLaunchKernelGGL(acx::pool_median_kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream,
                               d_raw.get(), raw_offsets[t0], d_roff.get(), d_poff.get(), n_tracks, poff[t0], poff[t1], fac, d_pooled.get());
            ACX_HIP(c, hipGetLastError());
            ACX_HIP(c, hipMemcpyAsync(pooled.data() + poff[t0] * 12, d_pooled, sizeof(float) * npool * 12, hipMemcpyDeviceToHost, c->stream));
            ACX_HIP(c, hipStreamSynchronize(c->stream));
            return ACX_OK;
        });
    if (rc != ACX_OK) return rc;
    if (pooled_offsets_out) memcpy(pooled_offsets_out, poff.data(), sizeof(int64_t) * (n_tracks + 1));
    return upload_pool_impl(c, pooled.data(), poff.data(), n_tracks, dim);
}

int acx_download_pool(acx_ctx *c, float *frames, int64_t capacity)
{
    if (!c) return ACX_ERR_INVALID;
    if (!c->d_frames0) return fail(c, ACX_ERR_STATE, "download_pool: feature pool not uploaded");
    const int64_t need = c->h_off0[c->n_tracks] * c->dim;
    if (!frames || capacity < need) return fail(c, ACX_ERR_INVALID, "download_pool: buffer too small");
    ACX_HIP(c, hipSetDevice(c->device));
    ACX_HIP(c, hipMemcpy(frames, c->d_frames0, sizeof(float) * need, hipMemcpyDeviceToHost));
    return ACX_OK;
}

void acx_serra09_default_params(acx_serra09_params *p)
{
    if (!p) return;
    p->m = 9; p->tau = 1; p->kappa = 0.095f; p->oti = 1; p->gamma_o = 0.5f; p->gamma_e = 0.5f;
    p->embed_full = 0; p->pct_mode = 0; p->oti_target = 0; p->dp_start = 2; p->inclusive = 1; p->dmax = 0; p->arith = ACX_ARITH_EXACT;
}

int32_t acx_serra09_embed_len(int32_t T, const acx_serra09_params *p)
{
    if (!p || p->m < 1 || p->tau < 1) return 0;
    return acx::serra09_embed_len(T, p->m, p->tau, p->embed_full);
}

int acx_serra09_pairs(acx_ctx *c, const int32_t *pairs, int64_t K, const acx_serra09_params *params, float *out)
{
    if (!c) return ACX_ERR_INVALID;
    if (K < 0 || (K > 0 && (!pairs || !out)) || !params) return fail(c, ACX_ERR_INVALID, "serra09_pairs: bad argument");
    if (K == 0) return ACX_OK;
    return run_serra09(c, pairs, K, *params, out, nullptr);
}

int acx_chenfusion_pairs(acx_ctx *c, const int32_t *pairs, int64_t K, const acx_serra09_params *params, float *out)
{
    if (!c) return ACX_ERR_INVALID;
    if (K < 0 || (K > 0 && (!pairs || !out)) || !params) return fail(c, ACX_ERR_INVALID, "chenfusion_pairs: bad argument");
    if (K == 0) return ACX_OK;
    return run_serra09(c, pairs, K, *params, out, nullptr, true);
}

int acx_serra09_debug_pair(acx_ctx *c, int32_t i, int32_t j, const acx_serra09_params *params,
                           float *d2, float *epsq, float *epsr, float *thrq, float *thrr,
                           int32_t *oti, float *score, int32_t *dims)
{
    if (!c) return ACX_ERR_INVALID;
    if (!params) return fail(c, ACX_ERR_INVALID, "serra09_debug_pair: bad argument");
    int32_t pr[2] = {i, j};
    float s = 0.0f;
    DebugOut dbg{d2, epsq, epsr, thrq, thrr, oti, dims};
    int rc = run_serra09(c, pr, 1, *params, &s, &dbg);
    if (rc == ACX_OK && score) *score = s;
    return rc;
}

// Would run_serra09 take the whole list in ONE batch?  The plan's own packing from pair 0, for the product path (no D2 in the
// scratch but for streaming-class pairs), on the uploaded pool's lengths (ensure_tau has not run yet).  A list the run would refuse
// (index, length, scratch limit) answers true: the run itself reports it, before its first launch.
static bool serra09_one_batch(const acx_ctx *c, const int32_t *pairs, int64_t K, const acx_serra09_params &p)
{
    const acx::Serra09Lengths len{c->h_off0.data(), c->n_tracks, p.tau};
    const int64_t limit_floats = scratch_limit_bytes(c) / 4;
    int64_t bad = 0;
    if (acx::serra09_check_pairs(len, pairs, K, p, false, limit_floats, &bad) != ACX_OK) return true;
    std::vector<PairDesc> pd;
    acx::Serra09Arena used;
    return acx::serra09_pack_batch(len, pairs, 0, K, p, false, limit_floats, pd, used) == K;
}

int acx_serra09_debug_bits(acx_ctx *c, const int32_t *pairs, int64_t K, const acx_serra09_params *params, float *scores,
                           uint8_t *R_out, int64_t *outside)
{
    if (!c) return ACX_ERR_INVALID;
    if (K < 0 || (K > 0 && (!pairs || !scores || !R_out)) || !params) return fail(c, ACX_ERR_INVALID, "serra09_debug_bits: bad argument");
    if (outside) *outside = 0;
    if (K == 0) return ACX_OK;
    if (!c->d_frames0) return fail(c, ACX_ERR_STATE, "serra09: feature pool not uploaded (acx_upload_pool)");
    int rc = check_params(c, *params);
    if (rc != ACX_OK) return rc;
    if (!serra09_one_batch(c, pairs, K, *params))
        return fail(c, ACX_ERR_UNSUPPORTED, "serra09_debug_bits: the pair list does not fit one batch");
    // the product call itself: no debug flag reaches a kernel, the sweeps keep their stream, the batch keeps its class sort
    if ((rc = run_serra09(c, pairs, K, *params, scores, nullptr)) != ACX_OK) return rc;
    // one batch: slot 0 still holds its descriptors (sorted by class key) and perm[k2] = position in `pairs` of sorted pair k2;
    // collect_slot has waited for the sweeps, which waited for every band kernel
    const Serra09Slot &S = c->slot[0];
    if (S.B != K) return fail(c, ACX_ERR_STATE, "serra09_debug_bits: the run took more than one batch");
    int64_t words = 0;
    std::vector<int64_t> offR((size_t)K + 1, 0);
    for (int k2 = 0; k2 < S.B; ++k2) {
        const PairDesc &d = S.pd[k2];
        words = std::max<int64_t>(words, d.offT + (int64_t)d.Mq * d.nw);
        offR[(size_t)S.perm[k2] + 1] = (int64_t)d.Mq * d.Mr;
    }
    for (int64_t k = 0; k < K; ++k) offR[k + 1] += offR[k];
    std::vector<unsigned long long> h((size_t)words);
    ACX_HIP(c, hipMemcpy(h.data(), c->d_bits, sizeof(unsigned long long) * (size_t)words, hipMemcpyDeviceToHost));
    // the inverse of acx_qmax_binary's packing: bit b of word t of row i = column 64 t + b - 7 + (i & 7)
    int64_t out_bits = 0;
    for (int k2 = 0; k2 < S.B; ++k2) {
        const PairDesc &d = S.pd[k2];
        uint8_t *R = R_out + offR[S.perm[k2]];
        for (int i = 0; i < d.Mq; ++i) {
            const int c0 = (i & (acx::BAND - 1)) - (acx::BAND - 1);
            const unsigned long long *row = h.data() + d.offT + (int64_t)i * d.nw;
            uint8_t *Ri = R + (int64_t)i * d.Mr;
            memset(Ri, 0, (size_t)d.Mr);
            for (int t = 0; t < d.nw; ++t) {
                unsigned long long wd = row[t];
                while (wd) {
                    const int j = 64 * t + __builtin_ctzll(wd) + c0;
                    wd &= wd - 1;
                    if (j >= 0 && j < d.Mr) Ri[j] = 1; else ++out_bits;
                }
            }
        }
    }
    if (outside) *outside = out_bits;
    return ACX_OK;
}

// A caller's binary M x N recurrence plot as the one pair of a Serra09 batch: checked (`who` names the entry point), packed into `words`
// in the pipeline's bitmap layout -- word t of row i = columns [64 t - 7 + (i & 7), +64) -- and queued for d_bits, with its descriptor
// `d` for slot 0.  The queued copies read `d` and `words`: both are the caller's, to keep until the stream is idle.
static int stage_serra09_plot(acx_ctx *c, const std::string &who, const uint8_t *R, int M, int N, PairDesc &d, std::vector<unsigned long long> &words)
{
    memset(&d, 0, sizeof(d));
    d.Mq = M; d.Mr = N; d.Tq = M; d.Tr = N;
    d.pitchD = round_up(N, 64); d.pitchT = 0;
    d.nw = acx::serra09_tiles(N);
    words.assign((size_t)M * d.nw, 0ull);
    for (int i = 0; i < M; ++i) {
        const int c0 = (i & (acx::BAND - 1)) - (acx::BAND - 1);
        for (int j = 0; j < N; ++j) {
            const uint8_t v = R[(size_t)i * N + j];
            if (v > 1) return fail(c, ACX_ERR_INVALID, who + ": non-binary elements found in input");
            if (v) { const int pos = j - c0; words[(size_t)i * d.nw + (pos >> 6)] |= 1ull << (pos & 63); }
        }
    }
    int rc;
    if ((rc = ensure(c, c->d_bits, words.size())) != ACX_OK) return rc;
    if ((rc = ensure(c, c->slot[0].d_pd, (size_t)1)) != ACX_OK) return rc;
    ACX_HIP(c, hipMemcpyAsync(c->d_bits, words.data(), sizeof(unsigned long long) * words.size(), hipMemcpyHostToDevice, c->stream));
    ACX_HIP(c, hipMemcpyAsync(c->slot[0].d_pd, &d, sizeof(d), hipMemcpyHostToDevice, c->stream));
    return ACX_OK;
}

int acx_qmax_binary(acx_ctx *c, const uint8_t *R, int32_t M, int32_t N, const acx_serra09_params *params, float *score)
{
    if (!c) return ACX_ERR_INVALID;
    PairDesc d;
    std::vector<unsigned long long> words;
    return guarded(c, [&]() -> int {
        if (!R || !params || !score || M < 1 || N < 1) return fail(c, ACX_ERR_INVALID, "qmax_binary: bad argument");
        if (params->dp_start != 2 && params->dp_start != 3) return fail(c, ACX_ERR_INVALID, "qmax_binary: dp_start must be 2 or 3");
        if (!(params->gamma_o >= 0.0f) || !(params->gamma_e >= 0.0f)) return fail(c, ACX_ERR_INVALID, "qmax_binary: gammas must be >= 0");
        ACX_HIP(c, hipSetDevice(c->device));
        int rc;
        Serra09Slot &S = c->slot[0];
        if ((rc = stage_serra09_plot(c, "qmax_binary", R, M, N, d, words)) != ACX_OK) return rc;
        if ((rc = ensure(c, c->d_scratch, (size_t)8 * M + 16)) != ACX_OK) return rc;     // strip records of the long DP
        if ((rc = ensure(c, S.d_out, (size_t)2)) != ACX_OK) return rc;
        // (one pair of any shape: the class of its longer side, never packed)
        launch_qmax_sweep(c->stream, S.d_pd, 1, c->d_bits, c->d_scratch, S.d_out, 1, params->gamma_o, params->gamma_e, params->dp_start,
                          params->dmax != 0, acx::serra09_sweep(acx::serra09_row_class(std::max(M, N))).cols, 1);
        ACX_HIP(c, hipGetLastError());
        ACX_HIP(c, hipMemcpyAsync(score, S.d_out, sizeof(float), hipMemcpyDeviceToHost, c->stream));
        ACX_HIP(c, hipStreamSynchronize(c->stream));
        return ACX_OK;
    });
}

int acx_serra09_align(acx_ctx *c, const int32_t *pairs, int64_t K, const acx_serra09_params *params, acx_alignment *out)
{
    if (!c) return ACX_ERR_INVALID;
    if (K < 0 || (K > 0 && (!pairs || !out)) || !params) return fail(c, ACX_ERR_INVALID, "serra09_align: bad argument");
    if (params->dmax != 0) return fail(c, ACX_ERR_UNSUPPORTED, "serra09_align: the Qmax alignment only (params->dmax must be 0)");
    if (K == 0) return ACX_OK;
    return run_serra09(c, pairs, K, *params, nullptr, nullptr, false, nullptr, out);
}

// The locating sweep alone on a given plot (acx_qmax_locate_binary; `dmax`: acx_dmax_locate_binary); `who` names the entry point in errors.
static int locate_binary(acx_ctx *c, const uint8_t *R, int32_t M, int32_t N, const acx_serra09_params *params, acx_alignment *out, bool dmax,
                         const std::string &who)
{
    PairDesc d;
    std::vector<unsigned long long> words;
    static const int64_t seam_off = 0;
    return guarded(c, [&]() -> int {
        if (params->dp_start != 2 && params->dp_start != 3) return fail(c, ACX_ERR_INVALID, who + ": dp_start must be 2 or 3");
        if (!(params->gamma_o >= 0.0f) || !(params->gamma_e >= 0.0f)) return fail(c, ACX_ERR_INVALID, who + ": gammas must be >= 0");
        if ((int64_t)M * N + acx::LOC_STRIP >= ((int64_t)1 << 32)) return fail(c, ACX_ERR_UNSUPPORTED, who + ": the plot has 2^32 cells or more");
        ACX_HIP(c, hipSetDevice(c->device));
        int rc;
        Serra09Slot &S = c->slot[0];
        if ((rc = stage_serra09_plot(c, who, R, M, N, d, words)) != ACX_OK) return rc;
        if ((rc = ensure(c, c->d_seam, (size_t)std::max<int64_t>(acx::loc_seam_records(M, N, params->dp_start), 1))) != ACX_OK) return rc;
        if ((rc = ensure(c, S.d_al, (size_t)1)) != ACX_OK) return rc;
        if ((rc = ensure(c, S.d_seam_off, (size_t)1)) != ACX_OK) return rc;
        ACX_HIP(c, hipMemcpyAsync(S.d_seam_off, &seam_off, sizeof(seam_off), hipMemcpyHostToDevice, c->stream));
        if (dmax) launch_dmax_locate(c->stream, S.d_pd, 1, c->d_bits, c->d_seam, S.d_seam_off, S.d_al, params->gamma_o, params->gamma_e, params->dp_start);
        else launch_qmax_locate(c->stream, S.d_pd, 1, c->d_bits, c->d_seam, S.d_seam_off, S.d_al, params->gamma_o, params->gamma_e, params->dp_start);
        ACX_HIP(c, hipGetLastError());
        ACX_HIP(c, hipMemcpyAsync(out, S.d_al, sizeof(acx_alignment), hipMemcpyDeviceToHost, c->stream));
        ACX_HIP(c, hipStreamSynchronize(c->stream));
        return ACX_OK;
    });
}

int acx_qmax_locate_binary(acx_ctx *c, const uint8_t *R, int32_t M, int32_t N, const acx_serra09_params *params, acx_alignment *out)
{
    if (!c) return ACX_ERR_INVALID;
    if (!R || !params || !out || M < 1 || N < 1) return fail(c, ACX_ERR_INVALID, "qmax_locate_binary: bad argument");
    if (params->dmax != 0) return fail(c, ACX_ERR_UNSUPPORTED, "qmax_locate_binary: the Qmax alignment only (params->dmax must be 0)");
    return locate_binary(c, R, M, N, params, out, false, "qmax_locate_binary");
}

int acx_dmax_locate_binary(acx_ctx *c, const uint8_t *R, int32_t M, int32_t N, const acx_serra09_params *params, acx_alignment *out)
{
    if (!c) return ACX_ERR_INVALID;
    if (!R || !params || !out || M < 1 || N < 1) return fail(c, ACX_ERR_INVALID, "dmax_locate_binary: bad argument");
    return locate_binary(c, R, M, N, params, out, true, "dmax_locate_binary");
}

// no more cells than this in the paths of one pair's `per` records: a path has no more cells than its plot's shorter side, and the
// sections of a pair (per > 1) are row-disjoint with at most as many cells each as their box has rows (per == 1: min(Mq, Mr))
static int64_t path_cells_bound(int Mq, int Mr, int per)
{
    return std::min<int64_t>(Mq, (int64_t)per * std::min(Mq, Mr));
}

// What the path exports check before the first launch: the run's own checks of the list, in its order, and `cap` against the bound
// the host knows then -- the sum over the list of path_cells_bound(Mq_k, Mr_k, per) in embedded frames, `rule` in the message.
static int check_path_cap(acx_ctx *c, const std::string &who, const int32_t *pairs, int64_t K, const acx_serra09_params &params, int64_t cap,
                          int per, const char *rule)
{
    if (!c->d_frames0) return fail(c, ACX_ERR_STATE, "serra09: feature pool not uploaded (acx_upload_pool)");
    if (c->dim != acx::NBIN) return fail(c, ACX_ERR_INVALID, "serra09: pool dim must be 12");
    int rc = check_params(c, params);
    if (rc != ACX_OK) return rc;
    const acx::Serra09Lengths len{c->h_off0.data(), c->n_tracks, params.tau};
    if ((rc = validate_serra09_pairs(c, len, pairs, K, params, false, scratch_limit_bytes(c) / 4)) != ACX_OK) return rc;
    int64_t bound = 0;
    for (int64_t k = 0; k < K; ++k) {
        PairDesc d;
        acx::Serra09Need need;
        (void)acx::serra09_size_pair(len, pairs[2 * k], pairs[2 * k + 1], params, false, d, need);
        bound += path_cells_bound(d.Mq, d.Mr, per);
    }
    if (cap < bound)
        return fail(c, ACX_ERR_INVALID, who + ": cap " + std::to_string(cap) + " is too small: " + std::to_string(bound) +
                                            " cells required (the sum of " + rule + " over the list)");
    return ACX_OK;
}

// the paths of a run, one vector per record, packed behind one another: path_off[t + 1] = cells up to and including record t
static void pack_paths(const std::vector<std::vector<int32_t>> &paths, int64_t *path_off, int32_t *cells)
{
    int64_t n = 0;
    path_off[0] = 0;
    for (size_t t = 0; t < paths.size(); ++t) {
        if (!paths[t].empty()) memcpy(cells + 2 * n, paths[t].data(), sizeof(int32_t) * paths[t].size());
        n += (int64_t)paths[t].size() / 2;
        path_off[t + 1] = n;
    }
}

// acx_serra09_align_paths, and (`al_dmax`) plane 1 of acx_chenfusion_align_paths; `who` names the entry point in errors.
static int align_paths(acx_ctx *c, const int32_t *pairs, int64_t K, const acx_serra09_params *params, acx_alignment *out,
                       int64_t *path_off, int32_t *cells, int64_t cap, bool al_dmax, const std::string &who)
{
    if (K < 0 || (K > 0 && (!pairs || !out)) || !params || !path_off || cap < 0 || (cap > 0 && !cells))
        return fail(c, ACX_ERR_INVALID, who + ": bad argument");
    path_off[0] = 0;
    if (K == 0) return ACX_OK;
    // (no path has more cells than its plot's shorter side)
    int rc = check_path_cap(c, who, pairs, K, *params, cap, 1, "min(Mq, Mr)");
    if (rc != ACX_OK) return rc;
    std::vector<std::vector<int32_t>> paths((size_t)K);
    if ((rc = run_serra09(c, pairs, K, *params, nullptr, nullptr, false, nullptr, out, &paths, al_dmax)) != ACX_OK) return rc;
    pack_paths(paths, path_off, cells);
    return ACX_OK;
}

int acx_serra09_align_paths(acx_ctx *c, const int32_t *pairs, int64_t K, const acx_serra09_params *params, acx_alignment *out,
                            int64_t *path_off, int32_t *cells, int64_t cap)
{
    if (!c) return ACX_ERR_INVALID;
    if (params && params->dmax != 0) return fail(c, ACX_ERR_UNSUPPORTED, "serra09_align_paths: the Qmax alignment only (params->dmax must be 0)");
    return align_paths(c, pairs, K, params, out, path_off, cells, cap, false, "serra09_align_paths");
}

// LateFusionChen: the alignment of one of the two planes acx_chenfusion_pairs scores.  params->dmax is ignored,
// as there; plane 0 is acx_serra09_align* itself.
int acx_chenfusion_align(acx_ctx *c, const int32_t *pairs, int64_t K, const acx_serra09_params *params, int32_t plane, acx_alignment *out)
{
    if (!c) return ACX_ERR_INVALID;
    if (plane != 0 && plane != 1) return fail(c, ACX_ERR_INVALID, "chenfusion_align: plane must be 0 (qmax) or 1 (dmax)");
    if (K < 0 || (K > 0 && (!pairs || !out)) || !params) return fail(c, ACX_ERR_INVALID, "chenfusion_align: bad argument");
    acx_serra09_params p = *params;
    p.dmax = 0;
    if (plane == 0) return acx_serra09_align(c, pairs, K, &p, out);
    if (K == 0) return ACX_OK;
    return run_serra09(c, pairs, K, p, nullptr, nullptr, false, nullptr, out, nullptr, true);
}

int acx_chenfusion_align_paths(acx_ctx *c, const int32_t *pairs, int64_t K, const acx_serra09_params *params, int32_t plane, acx_alignment *out,
                               int64_t *path_off, int32_t *cells, int64_t cap)
{
    if (!c) return ACX_ERR_INVALID;
    if (plane != 0 && plane != 1) return fail(c, ACX_ERR_INVALID, "chenfusion_align_paths: plane must be 0 (qmax) or 1 (dmax)");
    if (!params) return fail(c, ACX_ERR_INVALID, "chenfusion_align_paths: bad argument");
    acx_serra09_params p = *params;
    p.dmax = 0;
    if (plane == 0) return acx_serra09_align_paths(c, pairs, K, &p, out, path_off, cells, cap);
    return align_paths(c, pairs, K, &p, out, path_off, cells, cap, true, "chenfusion_align_paths");
}

// acx_qmax_path_binary, and (`dmax`) acx_dmax_path_binary; `who` names the entry point in errors.
static int path_binary(acx_ctx *c, const uint8_t *R, int32_t M, int32_t N, const acx_serra09_params *params, acx_alignment *out,
                       int64_t *n_cells, int32_t *cells, int64_t cap, bool dmax, const std::string &who)
{
    return guarded(c, [&]() -> int {
        if (!R || !params || !out || !n_cells || M < 1 || N < 1 || cap < 0 || (cap > 0 && !cells)) return fail(c, ACX_ERR_INVALID, who + ": bad argument");
        if (cap < std::min(M, N))
            return fail(c, ACX_ERR_INVALID, who + ": cap " + std::to_string(cap) + " is too small: " + std::to_string(std::min(M, N)) +
                                                " cells required (min(M, N))");
        *n_cells = 0;
        // the locating sweep on the plot: it leaves the plot's bitmap in d_bits and its descriptor in slot 0, and the record is the box
        int rc = dmax ? acx_dmax_locate_binary(c, R, M, N, params, out) : acx_qmax_locate_binary(c, R, M, N, params, out);
        if (rc != ACX_OK) return rc;
        std::vector<int32_t> path;
        rc = run_qmax_paths(c, c->slot[0].d_pd, out, 1, params->gamma_o, params->gamma_e,
                            [&](int) -> std::vector<int32_t> & { return path; }, [](int) { return std::string("0"); }, dmax);
        if (rc != ACX_OK) return rc;
        if (!path.empty()) memcpy(cells, path.data(), sizeof(int32_t) * path.size());
        *n_cells = (int64_t)path.size() / 2;
        return ACX_OK;
    });
}

int acx_qmax_path_binary(acx_ctx *c, const uint8_t *R, int32_t M, int32_t N, const acx_serra09_params *params, acx_alignment *out,
                         int64_t *n_cells, int32_t *cells, int64_t cap)
{
    if (!c) return ACX_ERR_INVALID;
    if (params && params->dmax != 0) return fail(c, ACX_ERR_UNSUPPORTED, "qmax_path_binary: the Qmax alignment only (params->dmax must be 0)");
    return path_binary(c, R, M, N, params, out, n_cells, cells, cap, false, "qmax_path_binary");
}

// ---- every section of a pair ----
// The option checks of acx_serra09_align_sections / acx_qmax_sections_binary, before any launch.
static int check_section_opts(acx_ctx *c, const std::string &who, const acx_section_opts &o)
{
    if (o.max_sections < 1 || o.max_sections > acx::SEC_MAX)
        return fail(c, ACX_ERR_INVALID, who + ": max_sections must be in [1, " + std::to_string(acx::SEC_MAX) + "]");
    if (o.pad < 0) return fail(c, ACX_ERR_INVALID, who + ": pad must be >= 0");
    if (!(o.min_score > 1.0f)) return fail(c, ACX_ERR_INVALID, who + ": min_score must be > 1");
    if (!(o.min_ratio >= 0.0f && o.min_ratio <= 1.0f)) return fail(c, ACX_ERR_INVALID, who + ": min_ratio must be in [0, 1]");
    return ACX_OK;
}

int acx_serra09_align_sections(acx_ctx *c, const int32_t *pairs, int64_t K, const acx_serra09_params *params, const acx_section_opts *opts,
                               acx_alignment *out, int32_t *n_sections, int64_t *path_off, int32_t *cells, int64_t cap)
{
    if (!c) return ACX_ERR_INVALID;
    const std::string who = "serra09_align_sections";
    if (params && params->dmax != 0) return fail(c, ACX_ERR_UNSUPPORTED, who + ": the Qmax alignment only (params->dmax must be 0)");
    if (K < 0 || (K > 0 && (!pairs || !out || !n_sections)) || !params || !opts || (path_off == nullptr) != (cells == nullptr) || (cells && cap < 0))
        return fail(c, ACX_ERR_INVALID, who + ": bad argument");
    int rc = check_section_opts(c, who, *opts);
    if (rc != ACX_OK) return rc;
    const int S = opts->max_sections;
    if (path_off) path_off[0] = 0;
    if (K == 0) return ACX_OK;
    SectionRun sec{*opts, n_sections};
    if (!cells) return run_serra09(c, pairs, K, *params, nullptr, nullptr, false, nullptr, out, nullptr, false, &sec);
    if ((rc = check_path_cap(c, who, pairs, K, *params, cap, S, "min(Mq, max_sections * min(Mq, Mr))")) != ACX_OK) return rc;
    std::vector<std::vector<int32_t>> paths((size_t)K * S);
    if ((rc = run_serra09(c, pairs, K, *params, nullptr, nullptr, false, nullptr, out, &paths, false, &sec)) != ACX_OK) return rc;
    pack_paths(paths, path_off, cells);
    return ACX_OK;
}

int acx_qmax_sections_binary(acx_ctx *c, const uint8_t *R, int32_t M, int32_t N, const acx_serra09_params *params, const acx_section_opts *opts,
                             acx_alignment *out, int32_t *n_sections, int64_t *path_off, int32_t *cells, int64_t cap)
{
    if (!c) return ACX_ERR_INVALID;
    const std::string who = "qmax_sections_binary";
    if (params && params->dmax != 0) return fail(c, ACX_ERR_UNSUPPORTED, who + ": the Qmax alignment only (params->dmax must be 0)");
    PairDesc d;
    std::vector<unsigned long long> words;
    static const int64_t seam_off = 0;
    return guarded(c, [&]() -> int {
        if (!R || !params || !opts || !out || !n_sections || M < 1 || N < 1 || (path_off == nullptr) != (cells == nullptr) || (cells && cap < 0))
            return fail(c, ACX_ERR_INVALID, who + ": bad argument");
        int rc = check_section_opts(c, who, *opts);
        if (rc != ACX_OK) return rc;
        const int S = opts->max_sections;
        if (params->dp_start != 2 && params->dp_start != 3) return fail(c, ACX_ERR_INVALID, who + ": dp_start must be 2 or 3");
        if (!(params->gamma_o >= 0.0f) || !(params->gamma_e >= 0.0f)) return fail(c, ACX_ERR_INVALID, who + ": gammas must be >= 0");
        if ((int64_t)M * N + acx::LOC_STRIP >= ((int64_t)1 << 32)) return fail(c, ACX_ERR_UNSUPPORTED, who + ": the plot has 2^32 cells or more");
        if (cells && cap < path_cells_bound(M, N, S))
            return fail(c, ACX_ERR_INVALID, who + ": cap " + std::to_string(cap) + " is too small: " + std::to_string(path_cells_bound(M, N, S)) +
                                                " cells required (min(M, max_sections * min(M, N)))");
        ACX_HIP(c, hipSetDevice(c->device));
        Serra09Slot &S0 = c->slot[0];
        if ((rc = stage_serra09_plot(c, who, R, M, N, d, words)) != ACX_OK) return rc;
        if ((rc = ensure(c, c->d_seam, (size_t)std::max<int64_t>(acx::loc_seam_records(M, N, params->dp_start), 1))) != ACX_OK) return rc;
        if ((rc = ensure(c, S0.d_al, (size_t)S)) != ACX_OK) return rc;
        if ((rc = ensure(c, S0.d_nsec, (size_t)1)) != ACX_OK) return rc;
        if ((rc = ensure(c, S0.d_seam_off, (size_t)1)) != ACX_OK) return rc;
        ACX_HIP(c, hipMemcpyAsync(S0.d_seam_off, &seam_off, sizeof(seam_off), hipMemcpyHostToDevice, c->stream));
        {
            ProfScope ps(c, KS_SECTIONS, (int64_t)M * N);
            launch_qmax_sections(c->stream, S0.d_pd, 1, c->d_bits, c->d_seam, S0.d_seam_off, S0.d_al, S0.d_nsec, params->gamma_o, params->gamma_e,
                                 params->dp_start, *opts);
        }
        ACX_HIP(c, hipGetLastError());
        ACX_HIP(c, hipMemcpyAsync(out, S0.d_al, sizeof(acx_alignment) * S, hipMemcpyDeviceToHost, c->stream));
        ACX_HIP(c, hipMemcpyAsync(n_sections, S0.d_nsec, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        ACX_HIP(c, hipStreamSynchronize(c->stream));
        drain_profile(c);
        if (!cells) return ACX_OK;
        std::vector<std::vector<int32_t>> paths((size_t)S);
        rc = run_qmax_paths(c, S0.d_pd, out, 1, params->gamma_o, params->gamma_e,
                            [&](int k2) -> std::vector<int32_t> & { return paths[(size_t)k2]; }, [](int) { return std::string("0"); }, false, S);
        if (rc != ACX_OK) return rc;
        pack_paths(paths, path_off, cells);
        return ACX_OK;
    });
}

int acx_dmax_path_binary(acx_ctx *c, const uint8_t *R, int32_t M, int32_t N, const acx_serra09_params *params, acx_alignment *out,
                         int64_t *n_cells, int32_t *cells, int64_t cap)
{
    if (!c) return ACX_ERR_INVALID;
    return path_binary(c, R, M, N, params, out, n_cells, cells, cap, true, "dmax_path_binary");
}

int acx_upload_pool_f64(acx_ctx *c, const double *frames, const int64_t *offsets, int32_t n_tracks, int32_t dim)
{
    if (!c) return ACX_ERR_INVALID;
    c->nf_zeroed = 0;
    return upload_pool_f64_impl(c, frames, offsets, n_tracks, dim);
}

static int upload_pool_f64_impl(acx_ctx *c, const double *frames, const int64_t *offsets, int32_t n_tracks, int32_t dim)
{
    if (!frames || !offsets || n_tracks <= 0 || dim != 12) return fail(c, ACX_ERR_INVALID, "upload_pool_f64: bad argument (dim must be 12)");
    if (offsets[0] != 0) return fail(c, ACX_ERR_INVALID, "upload_pool_f64: offsets[0] must be 0");
    for (int i = 0; i < n_tracks; ++i)
        if (offsets[i + 1] < offsets[i]) return fail(c, ACX_ERR_INVALID, "upload_pool_f64: offsets must be non-decreasing");
    ACX_HIP(c, hipSetDevice(c->device));
    // the old pool goes first (two pools need not fit side by side); the new one is the context's once it is complete, so
    // whatever fails below leaves no pool and the next call says so (ACX_ERR_STATE)
    (void)c->d_frames64.reset(); (void)c->d_toff64.reset(); (void)c->d_prof64.reset(); (void)c->d_wn64.reset();
    c->wn64_L = 0;
    c->n_tracks64 = 0;
    const int64_t total = offsets[n_tracks];
    std::vector<double> cleaned;
    DeviceBuffer<double> d_frames, d_prof;
    DeviceBuffer<int64_t> d_toff;
    ACX_HIP(c, d_frames.grow((size_t)std::max<int64_t>(1, total) * 12));
    ACX_HIP(c, d_toff.grow((size_t)n_tracks + 1));
    ACX_HIP(c, hipMemcpy(d_frames, frames, sizeof(double) * total * 12, hipMemcpyHostToDevice));
    ACX_HIP(c, hipMemcpy(d_toff, offsets, sizeof(int64_t) * (n_tracks + 1), hipMemcpyHostToDevice));
    {
        const int64_t before = c->nf_zeroed;
        const int rc = scan_nonfinite(c, "upload_pool_f64", "frames", d_frames.get(), total * 12, 12, 0, d_toff.get(), n_tracks);
        if (rc != ACX_OK) return rc;
        if (c->nf_zeroed > before) {      // policy ZERO: the profile below sums what the device holds
            cleaned.resize((size_t)total * 12);
            ACX_HIP(c, hipMemcpy(cleaned.data(), d_frames, sizeof(double) * total * 12, hipMemcpyDeviceToHost));
            frames = cleaned.data();
        }
    }
    // per-track chroma profile: sum over time (np.sum(seq, 1), simple_silva.py:46-47)
    std::vector<double> prof((size_t)n_tracks * 12, 0.0);
    for (int t = 0; t < n_tracks; ++t)
        for (int64_t f = offsets[t]; f < offsets[t + 1]; ++f)
            for (int b = 0; b < 12; ++b) prof[(size_t)t * 12 + b] += frames[f * 12 + b];
    ACX_HIP(c, d_prof.grow(prof.size()));
    ACX_HIP(c, hipMemcpy(d_prof, prof.data(), sizeof(double) * prof.size(), hipMemcpyHostToDevice));
    c->h_off64.assign(offsets, offsets + n_tracks + 1);
    c->n_tracks64 = n_tracks;
    c->d_frames64 = std::move(d_frames); c->d_toff64 = std::move(d_toff); c->d_prof64 = std::move(d_prof);
    return ACX_OK;
}

int acx_simple_upload_raw_pool(acx_ctx *c, const float *raw, const int64_t *raw_offsets, int32_t n_tracks, int32_t dim,
                               int32_t win, int32_t skip, int32_t win_len_smooth, int64_t *pooled_offsets_out)
{
    if (!c) return ACX_ERR_INVALID;
    int rc;
    if ((rc = check_raw_args(c, "simple_upload_raw_pool", raw, raw_offsets, n_tracks, dim)) != ACX_OK) return rc;
    if (win < 1 || skip < 1 || win_len_smooth < 0) return fail(c, ACX_ERR_INVALID, "simple_upload_raw_pool: WIN, SKIP must be >= 1 and the smoothing length >= 0");
    if (win_len_smooth + 2 > acx::SIMPLE_PREP_MAXW) return fail(c, ACX_ERR_UNSUPPORTED, "simple_upload_raw_pool: smoothing windows above 14 are not supported on the device");
    ACX_HIP(c, hipSetDevice(c->device));
    c->nf_zeroed = 0;
    std::vector<int64_t> poff((size_t)n_tracks + 1, 0);
    for (int t = 0; t < n_tracks; ++t) {
        const int64_t n = (raw_offsets[t + 1] - raw_offsets[t]) / skip;          // int(T0 / SKIP), simple_silva.py:37
        poff[t + 1] = poff[t] + n;
    }
    // scipy.signal.get_window('hann', n, fftbins=False) / sum  (simple_silva.py:58-60)
    acx::SmoothWin sw;
    sw.nw = win_len_smooth + 2;
    {
        double sum = 0.0;
        for (int k = 0; k < sw.nw; ++k) {
            sw.w[k] = sw.nw > 1 ? 0.5 - 0.5 * std::cos(2.0 * M_PI * (double)k / (double)(sw.nw - 1)) : 1.0;
            sum += sw.w[k];
        }
        for (int k = 0; k < sw.nw; ++k) sw.w[k] /= sum;
    }
    const int64_t ptotal = poff[n_tracks];
    std::vector<double> feats((size_t)std::max<int64_t>(1, ptotal) * 12);
    DeviceBuffer<int64_t> d_roff, d_poff;
    DeviceBuffer<float> d_raw;                       // staging of one slice: grown as needed, reused by the next
    DeviceBuffer<double> d_feats;
    ACX_HIP(c, d_roff.grow((size_t)n_tracks + 1));
    ACX_HIP(c, d_poff.grow((size_t)n_tracks + 1));
    ACX_HIP(c, hipMemcpy(d_roff, raw_offsets, sizeof(int64_t) * (n_tracks + 1), hipMemcpyHostToDevice));
    ACX_HIP(c, hipMemcpy(d_poff, poff.data(), sizeof(int64_t) * (n_tracks + 1), hipMemcpyHostToDevice));
    const int64_t budget = raw_slice_bytes(c);
    rc = for_track_slices(
        n_tracks, 65535, [&](int t0, int t1) { return (raw_offsets[t1] - raw_offsets[t0]) * 12 * (int64_t)sizeof(float) <= budget; },
        [&](int t0, int t1) -> int {
            const int64_t nraw = raw_offsets[t1] - raw_offsets[t0], npool = poff[t1] - poff[t0];
            if (npool <= 0) return ACX_OK;
            ACX_HIP(c, d_raw.grow((size_t)nraw * 12));
            ACX_HIP(c, d_feats.grow((size_t)npool * 12));
            ACX_HIP(c, hipMemcpyAsync(d_raw, raw + raw_offsets[t0] * 12, sizeof(float) * nraw * 12, hipMemcpyHostToDevice, c->stream));
            const int rcs = scan_nonfinite(c, "simple_upload_raw_pool", "raw chroma", d_raw.get(), nraw * 12, 12, raw_offsets[t0], d_roff.get(), n_tracks);
            if (rcs != ACX_OK) return rcs;
            hipLaunchKernelGGL(acx::simple_prep_kernel, dim3((unsigned)(t1 - t0)), dim3(256), 0, c->stream,
                               d_raw.get(), raw_offsets[t0], d_roff.get(), d_poff.get(), t0, win, skip, sw, d_feats.get(), poff[t0]);
            ACX_HIP(c, hipGetLastError());
            ACX_HIP(c, hipMemcpyAsync(feats.data() + poff[t0] * 12, d_feats, sizeof(double) * npool * 12, hipMemcpyDeviceToHost, c->stream));
            ACX_HIP(c, hipStreamSynchronize(c->stream));
            return ACX_OK;
        });
    if (rc != ACX_OK) return rc;
    if (pooled_offsets_out) memcpy(pooled_offsets_out, poff.data(), sizeof(int64_t) * (n_tracks + 1));
    return upload_pool_f64_impl(c, feats.data(), poff.data(), n_tracks, 12);
}

int acx_download_pool_f64(acx_ctx *c, double *frames, int64_t capacity)
{
    if (!c) return ACX_ERR_INVALID;
    if (!c->d_frames64) return fail(c, ACX_ERR_STATE, "download_pool_f64: f64 feature pool not uploaded");
    const int64_t need = c->h_off64[c->n_tracks64] * 12;
    if (!frames || capacity < need) return fail(c, ACX_ERR_INVALID, "download_pool_f64: buffer too small");
    ACX_HIP(c, hipSetDevice(c->device));
    ACX_HIP(c, hipMemcpy(frames, c->d_frames64, sizeof(double) * need, hipMemcpyDeviceToHost));
    return ACX_OK;
}

int acx_simple_pairs(acx_ctx *c, const int32_t *pairs, int64_t K, int32_t sslen, int32_t oti, double *out)
{
    if (!c) return ACX_ERR_INVALID;
    if (K < 0 || (K > 0 && (!pairs || !out))) return fail(c, ACX_ERR_INVALID, "simple_pairs: bad argument");
    if (K == 0) return ACX_OK;
    if (!c->d_frames64) return fail(c, ACX_ERR_STATE, "simple_pairs: f64 feature pool not uploaded (acx_upload_pool_f64)");
    if (sslen < 1 || sslen > acx::SIMPLE_MAXL) return fail(c, ACX_ERR_UNSUPPORTED, "simple_pairs: SSLEN must be in 1..16 on the device");
    ACX_HIP(c, hipSetDevice(c->device));
    int maxn = 0;
    for (int64_t k = 0; k < K; ++k) {
        for (int s = 0; s < 2; ++s) {
            const int t = pairs[2 * k + s];
            if (t < 0 || t >= c->n_tracks64) return fail(c, ACX_ERR_INVALID, "simple_pairs: track index out of range in pair " + std::to_string(k));
            const int n = (int)(c->h_off64[t + 1] - c->h_off64[t]);
            if (n < sslen) return fail(c, ACX_ERR_SHORT, "simple_pairs: track shorter than SSLEN (pair " + std::to_string(k) + ")");
            if (n > acx::SIMPLE_MAXN) return fail(c, ACX_ERR_UNSUPPORTED, "simple_pairs: tracks with more than 6000 pooled frames are not supported on the device");
            maxn = std::max(maxn, n);
        }
    }
    const size_t smem = simple_smem(maxn);
    int rcw = ensure_winnorm(c, sslen);
    if (rcw != ACX_OK) return rcw;
    const int64_t chunk = 1 << 22;
    int rc;
    if ((rc = ensure(c, c->d_pairs, (size_t)2 * std::min(K, chunk))) != ACX_OK) return rc;
    if ((rc = ensure(c, c->d_out64, (size_t)std::min(K, chunk))) != ACX_OK) return rc;
    std::vector<int32_t> order, sorted, bucket;
    std::vector<double> tmp;
    for (int64_t k0 = 0; k0 < K; k0 += chunk) {
        const int n = (int)std::min(chunk, K - k0);
        // sorted by the second track (then the first): neighbouring waves share the frames of B (scalar cache)
        // (stable counting sort on the second index: O(n))
        order.resize(n);
        const int32_t *pp = pairs + 2 * k0;
        bucket.assign((size_t)c->n_tracks64 + 1, 0);
        for (int k = 0; k < n; ++k) ++bucket[(size_t)pp[2 * k + 1] + 1];
        for (int t = 0; t < c->n_tracks64; ++t) bucket[t + 1] += bucket[t];
        for (int k = 0; k < n; ++k) order[bucket[pp[2 * k + 1]]++] = k;
        sorted.resize((size_t)2 * n);
        for (int k = 0; k < n; ++k) { sorted[2 * k] = pp[2 * order[k]]; sorted[2 * k + 1] = pp[2 * order[k] + 1]; }
        ACX_HIP(c, hipMemcpyAsync(c->d_pairs, sorted.data(), sizeof(int32_t) * 2 * n, hipMemcpyHostToDevice, c->stream));
        {
            ProfScope ps(c, KS_SIMPLE, n);
            if ((rc = launch_simple_sslen(c, sslen, n, smem, oti)) != ACX_OK) return rc;
        }
        ACX_HIP(c, hipGetLastError());
        tmp.resize(n);
        ACX_HIP(c, hipMemcpyAsync(tmp.data(), c->d_out64, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
        ACX_HIP(c, hipStreamSynchronize(c->stream));
        for (int k = 0; k < n; ++k) out[k0 + order[k]] = tmp[k];
        drain_profile(c);
    }
    return ACX_OK;
}

static_assert(sizeof(acx_simple_alignment) == sizeof(acx::SimpleProfileRec) && offsetof(acx_simple_alignment, run_len) == offsetof(acx::SimpleProfileRec, run_len) &&
              offsetof(acx_simple_alignment, q_span) == offsetof(acx::SimpleProfileRec, q_span), "simple_profile_kernel writes acx_simple_alignment");

int acx_simple_profile(acx_ctx *c, const int32_t *pairs, int64_t K, int32_t sslen, int32_t oti, acx_simple_alignment *out,
                       int64_t *offsets, double *mp, int32_t *mpi, int64_t cap)
{
    if (!c) return ACX_ERR_INVALID;
    if (K < 0 || (K > 0 && (!pairs || !out)) || cap < 0) return fail(c, ACX_ERR_INVALID, "simple_profile: bad argument");
    const bool want = offsets || mp || mpi;
    if (want && !(offsets && mp && mpi))
        return fail(c, ACX_ERR_INVALID, "simple_profile: offsets, mp and mpi must all be given (the profiles) or all be NULL (the records alone)");
    if (K == 0) { if (want) offsets[0] = 0; return ACX_OK; }
    if (!c->d_frames64) return fail(c, ACX_ERR_STATE, "simple_profile: f64 feature pool not uploaded (acx_upload_pool_f64)");
    if (sslen < 1 || sslen > acx::SIMPLE_MAXL) return fail(c, ACX_ERR_UNSUPPORTED, "simple_profile: SSLEN must be in 1..16 on the device");
    ACX_HIP(c, hipSetDevice(c->device));
    int maxn = 0;
    for (int64_t k = 0; k < K; ++k) {
        for (int s = 0; s < 2; ++s) {
            const int t = pairs[2 * k + s];
            if (t < 0 || t >= c->n_tracks64) return fail(c, ACX_ERR_INVALID, "simple_profile: track index out of range in pair " + std::to_string(k));
            const int n = (int)(c->h_off64[t + 1] - c->h_off64[t]);
            if (n < sslen) return fail(c, ACX_ERR_SHORT, "simple_profile: track shorter than SSLEN (pair " + std::to_string(k) + ")");
            if (n > acx::SIMPLE_MAXN) return fail(c, ACX_ERR_UNSUPPORTED, "simple_profile: tracks with more than 6000 pooled frames are not supported on the device");
            maxn = std::max(maxn, n);
        }
    }
    auto rows = [&](int64_t k) { const int t = pairs[2 * k]; return (int64_t)(c->h_off64[t + 1] - c->h_off64[t]) - sslen + 1; };
    // a chunk's device profiles: 12 bytes per row (f64 value + int32 index), inside the scratch limit
    const int64_t row_limit = want ? scratch_limit_bytes(c) / 12 : 0;
    if (want) {
        int64_t need = 0;
        for (int64_t k = 0; k < K; ++k) need += rows(k);
        if (cap < need)
            return fail(c, ACX_ERR_INVALID, "simple_profile: cap " + std::to_string(cap) + " is too small: " + std::to_string(need) +
                                                " elements are required (the sum of ma over the list)");
        for (int64_t k = 0; k < K; ++k)
            if (rows(k) > row_limit)
                return fail(c, ACX_ERR_NOMEM, "simple_profile: the profile of pair " + std::to_string(k) + " (" + std::to_string(rows(k)) +
                                                  " rows) does not fit the scratch limit (acx_set_scratch_limit)");
    }
    const size_t smem = simple_profile_smem(maxn);
    int rc = ensure_winnorm(c, sslen);
    if (rc != ACX_OK) return rc;
    if (want) { offsets[0] = 0; for (int64_t k = 0; k < K; ++k) offsets[k + 1] = offsets[k] + rows(k); }
    const int64_t chunk = 1 << 22;
    std::vector<int32_t> order, sorted, bucket;
    std::vector<int64_t> poff;
    std::vector<acx::SimpleProfileRec> tmp;
    for (int64_t k0 = 0; k0 < K;) {
        // the caller's pairs k0 .. k0 + n - 1: as many as the pair limit and the profile buffer take (at least one: checked above)
        int n = 0;
        int64_t nrows = 0;
        while (k0 + n < K && n < chunk && (!want || nrows + rows(k0 + n) <= row_limit)) { nrows += rows(k0 + n); ++n; }
        if ((rc = ensure(c, c->d_pairs, (size_t)2 * n)) != ACX_OK) return rc;
        if ((rc = ensure(c, c->d_sprec, (size_t)n)) != ACX_OK) return rc;
        if (want) {
            if ((rc = ensure(c, c->d_spoff, (size_t)n)) != ACX_OK) return rc;
            if ((rc = ensure(c, c->d_spmp, (size_t)std::max<int64_t>(1, nrows))) != ACX_OK) return rc;
            if ((rc = ensure(c, c->d_spmpi, (size_t)std::max<int64_t>(1, nrows))) != ACX_OK) return rc;
        }
        // sorted by the second track as acx_simple_pairs sorts (stable counting sort); a pair's profile keeps its place in the
        // CALLER's order, so the chunk's buffer is a slice of the caller's and comes back in one copy
        order.resize(n);
        const int32_t *pp = pairs + 2 * k0;
        bucket.assign((size_t)c->n_tracks64 + 1, 0);
        for (int k = 0; k < n; ++k) ++bucket[(size_t)pp[2 * k + 1] + 1];
        for (int t = 0; t < c->n_tracks64; ++t) bucket[t + 1] += bucket[t];
        for (int k = 0; k < n; ++k) order[bucket[pp[2 * k + 1]]++] = k;
        sorted.resize((size_t)2 * n);
        for (int k = 0; k < n; ++k) { sorted[2 * k] = pp[2 * order[k]]; sorted[2 * k + 1] = pp[2 * order[k] + 1]; }
        ACX_HIP(c, hipMemcpyAsync(c->d_pairs, sorted.data(), sizeof(int32_t) * 2 * n, hipMemcpyHostToDevice, c->stream));
        if (want) {
            poff.resize(n);
            for (int k = 0; k < n; ++k) poff[k] = offsets[k0 + order[k]] - offsets[k0];
            ACX_HIP(c, hipMemcpyAsync(c->d_spoff, poff.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice, c->stream));
        }
        {
            ProfScope ps(c, KS_SIMPLEPROF, n);
            if ((rc = launch_simple_profile_sslen(c, sslen, n, smem, oti, want ? c->d_spoff.get() : nullptr)) != ACX_OK) return rc;
        }
        ACX_LAUNCHES_OK(c);
        tmp.resize(n);
        ACX_HIP(c, hipMemcpyAsync(tmp.data(), c->d_sprec, sizeof(acx::SimpleProfileRec) * n, hipMemcpyDeviceToHost, c->stream));
        if (want && nrows > 0) {
            ACX_HIP(c, hipMemcpyAsync(mp + offsets[k0], c->d_spmp, sizeof(double) * nrows, hipMemcpyDeviceToHost, c->stream));
            ACX_HIP(c, hipMemcpyAsync(mpi + offsets[k0], c->d_spmpi, sizeof(int32_t) * nrows, hipMemcpyDeviceToHost, c->stream));
        }
        ACX_HIP(c, hipStreamSynchronize(c->stream));
        for (int k = 0; k < n; ++k) memcpy(&out[k0 + order[k]], &tmp[k], sizeof(acx_simple_alignment));
        drain_profile(c);
        k0 += n;
    }
    return ACX_OK;
}

static void ef_free_pool(acx_ctx *c)
{
    for (int k = 0; k < 3; ++k) { (void)c->d_ef[k].reset(); (void)c->d_efs[k].reset(); (void)c->d_efsc[k].reset(); }
    for (int k = 0; k < 2; ++k) (void)c->d_efn[k].reset();
    (void)c->d_efmed.reset();
    (void)c->d_efoff.reset();
    c->ef_ntracks = 0;
    c->ef_open = 0;
}

// (Re)build the split pools the matrix-pipe GEMMs read from the f32 features: fmt 0 = three bf16 terms, fmt 1 = two
// fp16 terms of x / inv[row] (ACX_EF_GEMM_F16X2; inv = the row's own power-of-two scale).  The pool keeps ONE of them
// (69 GB at DA-TACOS size): switching between the modes re-splits.
static int ef_build_splits(acx_ctx *c, int fmt)
{
    const int64_t nb = c->h_efoff.empty() ? 0 : c->h_efoff.back();
    for (int k = 0; k < 3 && nb > 0; ++k) {
        if (c->ef_kp[k] == 0 || !c->d_efs[k]) continue;
        if (fmt == 1) {
            if (!c->d_efsc[k]) {
                ACX_HIP(c, c->d_efsc[k].grow((size_t)nb + 32));      // (+ slack: a group of 16 scales is read at once)
                ACX_HIP(c, hipMemsetAsync(c->d_efsc[k], 0, sizeof(float) * (nb + 32), c->stream));
            }
            hipLaunchKernelGGL(acx::ef_rowscale_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, c->stream, c->d_ef[k], c->d_efsc[k], nb, c->ef_dims[k]);
        }
        const int64_t nthr = nb * c->ef_kp[k];
        hipLaunchKernelGGL(acx::ef_split_bf16_kernel, dim3((unsigned)std::min<int64_t>((nthr + 255) / 256, 1 << 22)), dim3(256), 0, c->stream,
                           c->d_ef[k], c->d_efs[k], nb, c->ef_dims[k], c->ef_kp[k], k == 2 ? 1 : 0, fmt == 1 ? c->d_efsc[k] : (const float *)nullptr);
        ACX_HIP(c, hipGetLastError());
    }
    c->ef_split_fmt = fmt;
    return ACX_OK;
}

// The block features are on the device (d_ef[0..2], d_efmed): unit-norm chroma rows in place
// (X / XNorm with zero norms -> 1, cross_recurrence.py:66-71) and the squared row norms of the
// Euclidean features (np.sum(X**2, 1), :46; f64 accumulation), once per pool.
static int ef_norms_and_splits(acx_ctx *c, const int64_t *offsets, int32_t n_tracks, const int32_t *dims);

static int ef_finish_pool(acx_ctx *c, const int64_t *offsets, int32_t n_tracks, const int32_t *dims)
{
    const int rc = ef_norms_and_splits(c, offsets, n_tracks, dims);
    if (rc != ACX_OK) ef_free_pool(c);                // whatever failed: no pool, the next call says so (ACX_ERR_STATE)
    return rc;
}

static int ef_norms_and_splits(acx_ctx *c, const int64_t *offsets, int32_t n_tracks, const int32_t *dims)
{
    const int64_t nb = offsets[n_tracks];
    c->h_efoff.assign(offsets, offsets + n_tracks + 1);
    c->ef_ntracks = n_tracks;
    for (int k = 0; k < 3; ++k) c->ef_dims[k] = dims[k];
    ACX_HIP(c, c->d_efoff.grow((size_t)n_tracks + 1));
    ACX_HIP(c, hipMemcpy(c->d_efoff, offsets, sizeof(int64_t) * (n_tracks + 1), hipMemcpyHostToDevice));
    {
        static const char *what[3] = {"mfcc blocks", "ssm blocks", "chroma blocks"};
        for (int k = 0; k < 3; ++k) {
            const int rc = scan_nonfinite(c, "ef pool", what[k], c->d_ef[k].get(), nb * dims[k], dims[k], 0, c->d_efoff.get(), n_tracks);
            if (rc != ACX_OK) return rc;
        }
    }
    for (int k = 0; k < 2; ++k)
        ACX_HIP(c, c->d_efn[k].grow((size_t)nb + 32));      // (+ slack: the rectangle GEMM reads a whole group of 16 norms)
    if (nb > 0) {
        const unsigned g = (unsigned)((nb + 3) / 4);
        hipLaunchKernelGGL(acx::ef_rownorm_kernel, dim3(g), dim3(256), 0, c->stream, c->d_ef[2], nb, dims[2], 1, (float *)nullptr);
        for (int k = 0; k < 2; ++k)
            hipLaunchKernelGGL(acx::ef_rownorm_kernel, dim3(g), dim3(256), 0, c->stream, c->d_ef[k], nb, dims[k], 0, c->d_efn[k]);
        ACX_HIP(c, hipGetLastError());
    }
    // three-term bf16 splits (the operands of the bf16 GEMM kernels): the two Euclidean features as they are, the
    // normalised chroma rows bin-major (ef_gemm_rect_bf16x3_kernel<1>) when a block has a multiple of 8 frames
    for (int k = 0; k < 3; ++k) {
        c->ef_kp[k] = (dims[k] + acx::EFB_BK - 1) / acx::EFB_BK * acx::EFB_BK;
        if (k == 2 && dims[2] % 96 != 0) { c->ef_kp[2] = 0; continue; }
        const int64_t nel = std::max<int64_t>(1, nb) * 3 * c->ef_kp[k];
        ACX_HIP(c, c->d_efs[k].grow((size_t)nel));
    }
    {
        const int rc = ef_build_splits(c, c->ef_gemm == ACX_EF_GEMM_F16X2 ? 1 : 0);
        if (rc != ACX_OK) return rc;
    }
    ACX_HIP(c, hipStreamSynchronize(c->stream));
    return ACX_OK;
}

// The pool in slices of whole tracks (a DA-TACOS-sized collection is 56 GB of block features: the host need
// not hold it in one piece).  begin: sizes and allocation; tracks: one slice, from HOST or DEVICE memory
// (hipMemcpyDefault: features that are already on the device, e.g. in a torch tensor, stay there); end: the
// non-finite scan, norms and bf16 splits -- the pool cannot be used before.
int acx_set_ef_gemm(acx_ctx *c, int32_t mode)
{
    if (!c) return ACX_ERR_INVALID;
    if (mode == -1) mode = ACX_EF_GEMM_DEFAULT;
    if (mode != ACX_EF_GEMM_BF16X3 && mode != ACX_EF_GEMM_F32 && mode != ACX_EF_GEMM_BF16X3_PAIRWISE && mode != ACX_EF_GEMM_BF16X3_CHROMA_F32 &&
        mode != ACX_EF_GEMM_F16X2)
        return fail(c, ACX_ERR_INVALID, "set_ef_gemm: unknown mode");
    c->ef_gemm = mode;
    return ACX_OK;
}

int acx_set_ef_fuse(acx_ctx *c, int32_t mode)
{
    if (!c) return ACX_ERR_INVALID;
    if (mode != ACX_EF_FUSE_FAST && mode != ACX_EF_FUSE_EXACT) return fail(c, ACX_ERR_INVALID, "set_ef_fuse: unknown mode");
    c->ef_fuse = mode;
    return ACX_OK;
}

int acx_ef_pool_begin(acx_ctx *c, const int64_t *offsets, int32_t n_tracks, const int32_t *dims)
{
    if (!c) return ACX_ERR_INVALID;
    if (!offsets || !dims || n_tracks <= 0) return fail(c, ACX_ERR_INVALID, "ef_pool_begin: bad argument");
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 12 || dims[2] % 12 != 0)
        return fail(c, ACX_ERR_INVALID, "ef_pool_begin: dims must be positive and dims[2] a multiple of 12");
    if (offsets[0] != 0) return fail(c, ACX_ERR_INVALID, "ef_pool_begin: offsets[0] must be 0");
    for (int i = 0; i < n_tracks; ++i)
        if (offsets[i + 1] < offsets[i]) return fail(c, ACX_ERR_INVALID, "ef_pool_begin: offsets must be non-decreasing");
    ACX_HIP(c, hipSetDevice(c->device));
    ef_free_pool(c);
    c->nf_zeroed = 0;
    const int64_t nb = offsets[n_tracks];
    for (int k = 0; k < 3; ++k) {
        const hipError_t e = c->d_ef[k].grow((size_t)std::max<int64_t>(1, nb) * dims[k]);
        if (e != hipSuccess) { ef_free_pool(c); return fail(c, ACX_ERR_NOMEM, std::string("ef_pool_begin: the block features do not fit the device: ") + hipGetErrorString(e)); }
    }
    {
        const hipError_t e = c->d_efmed.grow((size_t)12 * n_tracks);
        if (e != hipSuccess) { ef_free_pool(c); ACX_HIP(c, e); }
    }
    c->h_efoff.assign(offsets, offsets + n_tracks + 1);
    for (int k = 0; k < 3; ++k) c->ef_dims[k] = dims[k];
    c->ef_open = n_tracks;
    c->ef_filled.assign((size_t)n_tracks, 0);          // the arrays come from hipMalloc: what _tracks never wrote is garbage
    return ACX_OK;
}

int acx_ef_pool_tracks(acx_ctx *c, int32_t first_track, int32_t count, const float *mfccs, const float *ssms, const float *chromas,
                       const double *chroma_med)
{
    if (!c) return ACX_ERR_INVALID;
    if (c->ef_open <= 0) return fail(c, ACX_ERR_STATE, "ef_pool_tracks: no pool is being filled (acx_ef_pool_begin)");
    if (first_track < 0 || count < 0 || (int64_t)first_track + count > c->ef_open || !chroma_med)
        return fail(c, ACX_ERR_INVALID, "ef_pool_tracks: bad argument");
    if (count == 0) return ACX_OK;
    const int64_t b0 = c->h_efoff[first_track], nb = c->h_efoff[first_track + count] - b0;
    const float *src[3] = {mfccs, ssms, chromas};
    ACX_HIP(c, hipSetDevice(c->device));
    for (int k = 0; k < 3 && nb > 0; ++k) {
        if (!src[k]) return fail(c, ACX_ERR_INVALID, "ef_pool_tracks: bad argument");
        ACX_HIP(c, hipMemcpy(c->d_ef[k] + b0 * c->ef_dims[k], src[k], sizeof(float) * nb * c->ef_dims[k], hipMemcpyDefault));
    }
    ACX_HIP(c, hipMemcpy(c->d_efmed + (size_t)12 * first_track, chroma_med, sizeof(double) * 12 * count, hipMemcpyDefault));
    std::fill(c->ef_filled.begin() + first_track, c->ef_filled.begin() + first_track + count, (uint8_t)1);
    return ACX_OK;
}

int acx_ef_pool_end(acx_ctx *c)
{
    if (!c) return ACX_ERR_INVALID;
    if (c->ef_open <= 0) return fail(c, ACX_ERR_STATE, "ef_pool_end: no pool is being filled (acx_ef_pool_begin)");
    const int n_tracks = c->ef_open;
    {   // every track must have been handed over: the pool stays open (the missing slices can still be supplied)
        int64_t missing = 0, first = -1;
        for (int i = 0; i < n_tracks; ++i)
            if (!c->ef_filled[(size_t)i]) { if (first < 0) first = i; ++missing; }
        if (missing)
            return fail(c, ACX_ERR_STATE, "ef_pool_end: " + std::to_string(missing) + " of " + std::to_string(n_tracks) +
                        " tracks were never handed over by acx_ef_pool_tracks (first: track " + std::to_string(first) +
                        "); the pool is still open");
    }
    c->ef_open = 0;
    c->ef_filled.clear();
    ACX_HIP(c, hipSetDevice(c->device));
    {   // the chroma medians: one row of 12 per track
        const int rc = scan_nonfinite<double>(c, "ef pool", "chroma median", c->d_efmed.get(), (int64_t)12 * n_tracks, 12, 0, nullptr, n_tracks);
        if (rc != ACX_OK) { ef_free_pool(c); return rc; }
    }
    const std::vector<int64_t> off = c->h_efoff;
    const int32_t dims[3] = {c->ef_dims[0], c->ef_dims[1], c->ef_dims[2]};
    return ef_finish_pool(c, off.data(), n_tracks, dims);
}

int acx_ef_upload_pool(acx_ctx *c, const float *mfccs, const float *ssms, const float *chromas,
                       const double *chroma_med, const int64_t *offsets, int32_t n_tracks, const int32_t *dims)
{
    if (!c) return ACX_ERR_INVALID;
    if (!mfccs || !ssms || !chromas || !chroma_med || !offsets || !dims || n_tracks <= 0)
        return fail(c, ACX_ERR_INVALID, "ef_upload_pool: bad argument");
    int rc = acx_ef_pool_begin(c, offsets, n_tracks, dims);
    if (rc == ACX_OK) rc = acx_ef_pool_tracks(c, 0, n_tracks, mfccs, ssms, chromas, chroma_med);
    if (rc == ACX_OK) rc = acx_ef_pool_end(c);
    else { ef_free_pool(c); c->ef_open = 0; }
    return rc;
}

// Block features of tracks [0, n_tracks) into fresh device arrays: the caller's, to move into the context or to let drop.
struct EfBlocks {
    DeviceBuffer<float> feat[3];         // mfcc / ssm / chroma block features
    DeviceBuffer<double> med;            // chroma median, 12 per track
};

// Everything about a raw-feature upload that the host can refuse, before anything is allocated or a pool dropped: the
// parameters, the offsets, negative onsets (numpy's slice would count them from the end; the device clamps) and blocks
// whose resize needs a wider Gaussian than ef_blocks_kernel holds (radius as efp_resize computes it).  Fills the
// block offsets.
static int ef_plan_blocks(acx_ctx *c, const char *who, const int64_t *coff, const int64_t *moff, int32_t ncoef, const int64_t *onsets,
                          const int64_t *ooff, int32_t n_tracks, const acx_ef_prep_params &pp, std::vector<int64_t> &boff)
{
    if (pp.blocksize < 1 || pp.mfccs_per_block < 2 || pp.chromas_per_block < 1 || ncoef < 1)
        return fail(c, ACX_ERR_INVALID, "ef block features: bad parameter");
    if (pp.mfccs_per_block > acx::EFP_MAXROWS || pp.chromas_per_block > acx::EFP_MAXROWS || ncoef > acx::EFP_MAXDIM ||
        pp.mfccs_per_block * ncoef > acx::EFP_MAXROWS * acx::EFP_MAXDIM || pp.chromas_per_block * 12 > acx::EFP_MAXROWS * acx::EFP_MAXDIM)
        return fail(c, ACX_ERR_UNSUPPORTED, "ef block features: at most 64 rows per block and 40 coefficients per frame on the device");
    boff.assign((size_t)n_tracks + 1, 0);
    for (int t = 0; t < n_tracks; ++t) {
        if (coff[t + 1] < coff[t] || moff[t + 1] < moff[t] || ooff[t + 1] < ooff[t])
            return fail(c, ACX_ERR_INVALID, "ef block features: offsets must be non-decreasing");
        const int64_t nbeat = ooff[t + 1] - ooff[t];
        boff[t + 1] = boff[t] + std::max<int64_t>(0, nbeat - pp.blocksize);
        const int64_t *on = onsets + ooff[t];
        for (int64_t k = 0; k < nbeat; ++k)
            if (on[k] < 0)
                return fail(c, ACX_ERR_INVALID, std::string(who) + ": track " + std::to_string(t) + " has a negative onset (" +
                            std::to_string(on[k]) + "); numpy's slice would count it from the end");
        const int64_t len[2] = {moff[t + 1] - moff[t], coff[t + 1] - coff[t]};
        const int rows[2] = {pp.mfccs_per_block, pp.chromas_per_block}, last[2] = {pp.blocksize - 1, pp.blocksize};
        static const char *what[2] = {"MFCCs", "chroma"};
        for (int64_t b = 0; b < boff[t + 1] - boff[t]; ++b)
            for (int k = 0; k < 2; ++k) {
                const int64_t i1 = std::min(on[b], len[k]), i2 = std::min(on[b + last[k]], len[k]), n = std::max<int64_t>(0, i2 - i1);
                const double factor = (double)n / (double)rows[k], sigma = factor > 1.0 ? (factor - 1.0) * 0.5 : 0.0;
                if (4.0 * sigma + 0.5 >= (double)(acx::EFP_MAXRAD + 1))
                    return fail(c, ACX_ERR_UNSUPPORTED, "ef block features: block " + std::to_string(b) + " of track " + std::to_string(t) + " spans " +
                                std::to_string(n) + " frames of " + what[k] + ": its resize to " + std::to_string(rows[k]) +
                                " rows needs a Gaussian of radius " + std::to_string((int64_t)(4.0 * sigma + 0.5)) + ", at most " +
                                std::to_string(acx::EFP_MAXRAD) + " on the device");
            }
    }
    return ACX_OK;
}

// `boff`: the block offsets of ef_plan_blocks, which has passed.
static int ef_build_blocks(acx_ctx *c, const float *chroma, const int64_t *coff, const float *mfcc, const int64_t *moff,
                           int32_t ncoef, const int64_t *onsets, const int64_t *ooff, int32_t n_tracks,
                           const acx_ef_prep_params &pp, const std::vector<int64_t> &boff, EfBlocks &out)
{
    const int64_t nb = boff[n_tracks];
    const int dims[3] = {pp.mfccs_per_block * ncoef, pp.mfccs_per_block * (pp.mfccs_per_block - 1) / 2, pp.chromas_per_block * 12};
    for (int k = 0; k < 3; ++k) ACX_HIP(c, out.feat[k].grow((size_t)std::max<int64_t>(1, nb) * dims[k]));
    ACX_HIP(c, out.med.grow((size_t)12 * n_tracks));
    DeviceBuffer<float> d_ch, d_mf;                  // staging of one slice: grown as needed, reused by the next
    DeviceBuffer<int64_t> d_on, d_coff, d_moff, d_ooff, d_boff;
    const int64_t budget = raw_slice_bytes(c);
    auto slice_bytes = [&](int a, int b2) { return ((coff[b2] - coff[a]) * 12 + (moff[b2] - moff[a]) * ncoef) * (int64_t)sizeof(float); };
    return for_track_slices(
        n_tracks, 65535, [&](int t0, int t1) { return slice_bytes(t0, t1) <= budget; },
        [&](int t0, int t1) -> int {
            const int nt = t1 - t0;
            const int64_t nch = coff[t1] - coff[t0], nmf = moff[t1] - moff[t0], non = ooff[t1] - ooff[t0], nbs = boff[t1] - boff[t0];
            std::vector<int64_t> lc(nt + 1), lm(nt + 1), lo(nt + 1), lb(nt + 1);
            for (int t = 0; t <= nt; ++t) {
                lc[t] = coff[t0 + t] - coff[t0]; lm[t] = moff[t0 + t] - moff[t0];
                lo[t] = ooff[t0 + t] - ooff[t0]; lb[t] = boff[t0 + t] - boff[t0];
            }
            ACX_HIP(c, d_ch.grow((size_t)std::max<int64_t>(1, nch) * 12));
            ACX_HIP(c, d_mf.grow((size_t)std::max<int64_t>(1, nmf) * ncoef));
            ACX_HIP(c, d_on.grow((size_t)std::max<int64_t>(1, non)));
            for (DeviceBuffer<int64_t> *b : {&d_coff, &d_moff, &d_ooff, &d_boff}) ACX_HIP(c, b->grow((size_t)nt + 1));
            ACX_HIP(c, hipMemcpyAsync(d_ch, chroma + coff[t0] * 12, sizeof(float) * nch * 12, hipMemcpyHostToDevice, c->stream));
            ACX_HIP(c, hipMemcpyAsync(d_mf, mfcc + moff[t0] * ncoef, sizeof(float) * nmf * ncoef, hipMemcpyHostToDevice, c->stream));
            ACX_HIP(c, hipMemcpyAsync(d_on, onsets + ooff[t0], sizeof(int64_t) * non, hipMemcpyHostToDevice, c->stream));
            ACX_HIP(c, hipMemcpyAsync(d_coff, lc.data(), sizeof(int64_t) * (nt + 1), hipMemcpyHostToDevice, c->stream));
            ACX_HIP(c, hipMemcpyAsync(d_moff, lm.data(), sizeof(int64_t) * (nt + 1), hipMemcpyHostToDevice, c->stream));
            ACX_HIP(c, hipMemcpyAsync(d_ooff, lo.data(), sizeof(int64_t) * (nt + 1), hipMemcpyHostToDevice, c->stream));
            ACX_HIP(c, hipMemcpyAsync(d_boff, lb.data(), sizeof(int64_t) * (nt + 1), hipMemcpyHostToDevice, c->stream));
            // NaN MFCCs count as 0 like in the reference (earlyfusion_traile.py:105); anything else non-finite follows the policy
            // (the host offset tables above are pageable: their copies are staged before the calls return)
            int rcs = scan_nonfinite(c, "ef block features", "raw chroma", d_ch.get(), nch * 12, 12, 0, d_coff.get(), nt, false, t0);
            if (rcs == ACX_OK) rcs = scan_nonfinite(c, "ef block features", "MFCCs", d_mf.get(), nmf * ncoef, ncoef, 0, d_moff.get(), nt, true, t0);
            if (rcs != ACX_OK) return rcs;
            if (nbs > 0) {
                acx::EfPrepParams kp{pp.blocksize, pp.mfccs_per_block, pp.chromas_per_block, ncoef};
                hipLaunchKernelGGL(acx::ef_blocks_kernel, dim3((unsigned)nbs), dim3(256), 0, c->stream,
                                   d_ch.get(), d_coff.get(), d_mf.get(), d_moff.get(), d_on.get(), d_ooff.get(), d_boff.get(), nt, kp,
                                   out.feat[0] + boff[t0] * dims[0], out.feat[1] + boff[t0] * dims[1], out.feat[2] + boff[t0] * dims[2]);
            }
            hipLaunchKernelGGL(acx::ef_chroma_median_kernel, dim3(nt, 12), dim3(64), 0, c->stream, d_ch.get(), d_coff.get(), out.med + (size_t)t0 * 12);
            ACX_HIP(c, hipGetLastError());
            ACX_HIP(c, hipStreamSynchronize(c->stream));
            return ACX_OK;
        });
}

static int ef_check_raw(acx_ctx *c, const char *who, const float *chroma, const float *mfcc, const int64_t *onsets,
                        const acx_ef_prep_params *prep)
{
    if (!chroma || !mfcc || !onsets || !prep) return fail(c, ACX_ERR_INVALID, std::string(who) + ": bad argument");
    return ACX_OK;
}

int acx_ef_block_features(acx_ctx *c, const float *chroma, int64_t n_chroma, const float *mfcc, int64_t n_mfcc, int32_t ncoef,
                          const int64_t *onsets, int32_t n_beats, const acx_ef_prep_params *prep, float *mfccs, float *ssms,
                          float *chromas, double *chroma_med)
{
    if (!c) return ACX_ERR_INVALID;
    int rc = ef_check_raw(c, "ef_block_features", chroma, mfcc, onsets, prep);
    if (rc != ACX_OK) return rc;
    if (n_chroma < 0 || n_mfcc < 0 || n_beats < 0) return fail(c, ACX_ERR_INVALID, "ef_block_features: bad argument");
    const int64_t coff[2] = {0, n_chroma}, moff[2] = {0, n_mfcc}, ooff[2] = {0, n_beats};
    std::vector<int64_t> boff;
    if ((rc = ef_plan_blocks(c, "ef_block_features", coff, moff, ncoef, onsets, ooff, 1, *prep, boff)) != ACX_OK) return rc;
    ACX_HIP(c, hipSetDevice(c->device));
    c->nf_zeroed = 0;
    EfBlocks blocks;
    if ((rc = ef_build_blocks(c, chroma, coff, mfcc, moff, ncoef, onsets, ooff, 1, *prep, boff, blocks)) != ACX_OK) return rc;
    const int64_t nb = boff[1];
    const int dims[3] = {prep->mfccs_per_block * ncoef, prep->mfccs_per_block * (prep->mfccs_per_block - 1) / 2, prep->chromas_per_block * 12};
    float *dst[3] = {mfccs, ssms, chromas};
    for (int k = 0; k < 3; ++k)
        if (dst[k] && nb > 0) ACX_HIP(c, hipMemcpy(dst[k], blocks.feat[k], sizeof(float) * nb * dims[k], hipMemcpyDeviceToHost));
    if (chroma_med) ACX_HIP(c, hipMemcpy(chroma_med, blocks.med, sizeof(double) * 12, hipMemcpyDeviceToHost));
    return ACX_OK;
}

int acx_ef_upload_raw_pool(acx_ctx *c, const float *chroma, const int64_t *chroma_offsets, const float *mfcc,
                           const int64_t *mfcc_offsets, int32_t ncoef, const int64_t *onsets, const int64_t *onset_offsets,
                           int32_t n_tracks, const acx_ef_prep_params *prep, int64_t *block_offsets_out)
{
    if (!c) return ACX_ERR_INVALID;
    int rc = ef_check_raw(c, "ef_upload_raw_pool", chroma, mfcc, onsets, prep);
    if (rc != ACX_OK) return rc;
    if (!chroma_offsets || !mfcc_offsets || !onset_offsets || n_tracks <= 0) return fail(c, ACX_ERR_INVALID, "ef_upload_raw_pool: bad argument");
    std::vector<int64_t> boff;
    if ((rc = ef_plan_blocks(c, "ef_upload_raw_pool", chroma_offsets, mfcc_offsets, ncoef, onsets, onset_offsets, n_tracks, *prep, boff)) != ACX_OK)
        return rc;                                    // (the pool that is up stays as it is)
    ACX_HIP(c, hipSetDevice(c->device));
    ef_free_pool(c);
    c->nf_zeroed = 0;
    EfBlocks blocks;
    if ((rc = ef_build_blocks(c, chroma, chroma_offsets, mfcc, mfcc_offsets, ncoef, onsets, onset_offsets, n_tracks, *prep, boff,
                              blocks)) != ACX_OK) return rc;
    for (int k = 0; k < 3; ++k) c->d_ef[k] = std::move(blocks.feat[k]);
    c->d_efmed = std::move(blocks.med);
    const int32_t dims[3] = {prep->mfccs_per_block * ncoef, prep->mfccs_per_block * (prep->mfccs_per_block - 1) / 2, prep->chromas_per_block * 12};
    if (block_offsets_out) memcpy(block_offsets_out, boff.data(), sizeof(int64_t) * (n_tracks + 1));
    return ef_finish_pool(c, boff.data(), n_tracks, dims);
}

int acx_ef_download_pool(acx_ctx *c, float *mfccs, float *ssms, float *chromas, float *mfcc_sq, float *ssm_sq, double *chroma_med,
                         int64_t *offsets, int32_t *n_tracks, int32_t *dims)
{
    if (!c) return ACX_ERR_INVALID;
    if (!c->d_ef[0] || c->ef_open || c->ef_ntracks <= 0)
        return fail(c, ACX_ERR_STATE, "ef_download_pool: no finished block-feature pool (acx_ef_upload_pool / acx_ef_upload_raw_pool / acx_ef_pool_end)");
    const int64_t nb = c->h_efoff[(size_t)c->ef_ntracks];
    if (n_tracks) *n_tracks = c->ef_ntracks;
    if (dims) for (int k = 0; k < 3; ++k) dims[k] = c->ef_dims[k];
    if (offsets) memcpy(offsets, c->h_efoff.data(), sizeof(int64_t) * ((size_t)c->ef_ntracks + 1));
    ACX_HIP(c, hipSetDevice(c->device));
    float *dst[3] = {mfccs, ssms, chromas}, *sq[2] = {mfcc_sq, ssm_sq};
    for (int k = 0; k < 3; ++k)
        if (dst[k] && nb > 0) ACX_HIP(c, hipMemcpy(dst[k], c->d_ef[k], sizeof(float) * nb * c->ef_dims[k], hipMemcpyDeviceToHost));
    for (int k = 0; k < 2; ++k)
        if (sq[k] && nb > 0) ACX_HIP(c, hipMemcpy(sq[k], c->d_efn[k], sizeof(float) * nb, hipMemcpyDeviceToHost));
    if (chroma_med) ACX_HIP(c, hipMemcpy(chroma_med, c->d_efmed, sizeof(double) * 12 * c->ef_ntracks, hipMemcpyDeviceToHost));
    return ACX_OK;
}

int acx_earlyfusion_pairs(acx_ctx *c, const int32_t *pairs, int64_t K, const acx_ef_params *params, float *out)
{
    if (!c) return ACX_ERR_INVALID;
    if (K < 0 || (K > 0 && (!pairs || !out)) || !params) return fail(c, ACX_ERR_INVALID, "earlyfusion_pairs: bad argument");
    if (K == 0) return ACX_OK;
    // (indices are checked HERE, on the caller's list: the sorted copy below would name a pair by its sorted position; a track
    // without blocks is left to the run)
    int64_t upto;
    int rc = check_ef_pairs(c, pairs, K, &upto);
    if (rc != ACX_OK) return rc;
    // the list in run order (ef_run_order, ef_plan.hpp); one that is sorted already goes through as it is
    std::vector<int64_t> order;
    std::vector<int32_t> sp;
    if (acx::ef_run_order(pairs, K, order, sp)) return run_ef(c, pairs, K, *params, out, nullptr, nullptr, 0, 0);
    std::vector<float> so((size_t)4 * K);
    rc = run_ef(c, sp.data(), K, *params, so.data(), nullptr, nullptr, 0, 0);
    if (rc != ACX_OK) return rc;
    for (int64_t k = 0; k < K; ++k)
        for (int e = 0; e < 4; ++e) out[4 * order[(size_t)k] + e] = so[(size_t)4 * k + e];
    return ACX_OK;
}

int acx_ef_debug_pair(acx_ctx *c, int32_t i, int32_t j, const acx_ef_params *params, float *csm, float *fused,
                      float *scores, int32_t *oti)
{
    if (!c) return ACX_ERR_INVALID;
    if (!params) return fail(c, ACX_ERR_INVALID, "ef_debug_pair: bad argument");
    int32_t pr[2] = {i, j};
    float sc[4] = {0, 0, 0, 0};
    EfDebug dbg{csm, fused, oti};
    int rc = run_ef(c, pr, 1, *params, sc, &dbg, nullptr, 0, 0);
    if (rc == ACX_OK && scores) for (int k = 0; k < 4; ++k) scores[k] = sc[k];
    return rc;
}

int acx_ef_debug_pairs(acx_ctx *c, const int32_t *pairs, int64_t K, const acx_ef_params *params, int64_t which,
                       float *csm, float *fused, float *scores, int32_t *oti)
{
    if (!c) return ACX_ERR_INVALID;
    if (!params || !pairs || K < 1 || which < 0 || which >= K) return fail(c, ACX_ERR_INVALID, "ef_debug_pairs: bad argument");
    std::vector<float> sc((size_t)4 * K);
    EfDebug dbg{csm, fused, oti, which};
    const int rc = run_ef(c, pairs, K, *params, sc.data(), &dbg, nullptr, 0, 0);
    if (rc == ACX_OK && scores) memcpy(scores, sc.data(), sizeof(float) * 4 * (size_t)K);
    return rc;
}

int acx_ef_debug_bits(acx_ctx *c, const int32_t *pairs, int64_t K, const acx_ef_params *params, int64_t which,
                      uint32_t *bits, float *t, int32_t *jcut, float *r, float *cm, float *scores)
{
    if (!c) return ACX_ERR_INVALID;
    if (!params || !pairs || K < 1 || which < 0 || which >= K) return fail(c, ACX_ERR_INVALID, "ef_debug_bits: bad argument");
    // the list as acx_earlyfusion_pairs hands it to run_ef: sorted, the fused matrix not stored
    if (!acx::ef_in_run_order(pairs, K)) return fail(c, ACX_ERR_INVALID, "ef_debug_bits: the pair list must be sorted by (first track, second track)");
    std::vector<float> sc((size_t)4 * K);
    const EfStats st{bits, t, jcut, r, cm};
    EfDebug dbg{nullptr, nullptr, nullptr, which, &st};
    const int rc = run_ef(c, pairs, K, *params, sc.data(), &dbg, nullptr, 0, 0);
    if (rc == ACX_OK && scores) memcpy(scores, sc.data(), sizeof(float) * 4 * (size_t)K);
    return rc;
}

int acx_csm_debug_bits(acx_ctx *c, const float *D, int32_t M, int32_t N, double kappa, int32_t K,
                       uint32_t *bits, float *t, int32_t *jcut, float *r, float *score)
{
    if (!c) return ACX_ERR_INVALID;
    if (!D || M < 1 || N < 1) return fail(c, ACX_ERR_INVALID, "csm_debug_bits: bad argument");
    acx_ef_params p{kappa, K};
    float sc[4] = {0, 0, 0, 0};
    const EfStats st{bits, t, jcut, r, nullptr};
    EfDebug dbg{nullptr, nullptr, nullptr, 0, &st};
    const int rc = run_ef(c, nullptr, 1, p, sc, &dbg, D, M, N);
    if (rc == ACX_OK && score) *score = sc[0];
    return rc;
}

int acx_csm_binary_sw(acx_ctx *c, const float *D, int32_t M, int32_t N, double kappa, float *score)
{
    if (!c) return ACX_ERR_INVALID;
    if (!D || !score || M < 1 || N < 1) return fail(c, ACX_ERR_INVALID, "csm_binary_sw: bad argument");
    acx_ef_params p{kappa, 1};
    float sc[4] = {0, 0, 0, 0};
    const int rc = run_ef(c, nullptr, 1, p, sc, nullptr, D, M, N);
    if (rc == ACX_OK) *score = sc[0];
    return rc;
}

// A caller's binary M x N plot as the one pair `d` of an EarlyFusion batch, in one of the two layouts the kernels read.  `who` names the
// entry point where a value is neither 0 nor 1; empty: the reference's own text (alignment_tools.py:23), which acx_sw_binary and
// acx_sw_bits_binary report.  The queued copies read `d` and the host copy of the plot (`W` / `Cm`): both are the caller's, to keep
// until the stream is idle.
static int nonbinary(acx_ctx *c, const std::string &who)
{
    return fail(c, ACX_ERR_INVALID, who.empty() ? std::string("Non-binary elements found in input") : who + ": non-binary elements found in input");
}

// the bit words the selection kernels leave in d_efbits: bit j % 32 of word j / 32, M rows of pitchC / 32 words, pads zero
static int stage_ef_bit_plot(acx_ctx *c, const std::string &who, const uint8_t *B, int M, int N, acx::EfPair &d, std::vector<uint32_t> &W)
{
    d = ef_one_pair(M, N);
    const int words = d.pitchC / 32;
    W.assign((size_t)M * words, 0u);
    for (int i = 0; i < M; ++i)
        for (int j = 0; j < N; ++j) {
            const uint8_t b = B[(size_t)i * N + j];
            if (b > 1) return nonbinary(c, who);
            W[(size_t)i * words + (j >> 5)] |= (uint32_t)b << (j & 31);
        }
    int rc;
    ACX_HIP(c, hipSetDevice(c->device));
    if ((rc = ensure(c, c->d_efbits, W.size())) != ACX_OK) return rc;
    if ((rc = ensure(c, c->d_efpd, (size_t)1)) != ACX_OK) return rc;
    ACX_HIP(c, hipMemcpyAsync(c->d_efpd, &d, sizeof(d), hipMemcpyHostToDevice, c->stream));
    ACX_HIP(c, hipMemcpyAsync(c->d_efbits, W.data(), sizeof(uint32_t) * W.size(), hipMemcpyHostToDevice, c->stream));
    return ACX_OK;
}

// the float path's matrix, thresholds and tie columns: B = [C <= threshold] with C = 1 - B and threshold 0 in every row (written
// directly: the row-stat kernel would select by rank), every tie counted
static int stage_ef_float_plot(acx_ctx *c, const std::string &who, const uint8_t *B, int M, int N, acx::EfPair &d, std::vector<float> &Cm)
{
    d = ef_one_pair(M, N);
    Cm.resize((size_t)M * N);
    for (size_t k = 0; k < Cm.size(); ++k) {
        if (B[k] > 1) return nonbinary(c, who);
        Cm[k] = B[k] ? 0.0f : 1.0f;
    }
    int rc;
    ACX_HIP(c, hipSetDevice(c->device));
    if ((rc = ensure(c, c->d_scratch, (size_t)M * d.pitchC)) != ACX_OK) return rc;
    if ((rc = ensure(c, c->d_thr, (size_t)acx::ef_s_total(d))) != ACX_OK) return rc;
    if ((rc = ensure(c, c->d_efpd, (size_t)1)) != ACX_OK) return rc;
    ACX_HIP(c, hipMemcpyAsync(c->d_efpd, &d, sizeof(d), hipMemcpyHostToDevice, c->stream));
    ACX_HIP(c, hipMemcpy2DAsync(c->d_scratch, sizeof(float) * d.pitchC, Cm.data(), sizeof(float) * N, sizeof(float) * N, M,
                                hipMemcpyHostToDevice, c->stream));
    ACX_HIP(c, hipMemsetAsync(c->d_thr, 0, sizeof(float) * M, c->stream));
    ACX_HIP(c, hipMemsetAsync(c->d_thr + acx::ef_jcut_off(d, 0), 0x7f, sizeof(int) * M, c->stream));   // every tie counts
    return ACX_OK;
}

int acx_sw_binary(acx_ctx *c, const uint8_t *B, int32_t M, int32_t N, float *score)
{
    if (!c) return ACX_ERR_INVALID;
    acx::EfPair d;
    std::vector<float> Cm;
    float sc[4] = {0, 0, 0, 0};
    return guarded(c, [&]() -> int {
        if (!B || !score || M < 1 || N < 1) return fail(c, ACX_ERR_INVALID, "sw_binary: bad argument");
        int rc;
        if ((rc = stage_ef_float_plot(c, "", B, M, N, d, Cm)) != ACX_OK) return rc;
        if ((rc = ensure(c, c->d_out, (size_t)4)) != ACX_OK) return rc;
        if (N > acx::EF_MAXNB) hipLaunchKernelGGL(acx::sw_long_kernel, dim3(1, 1), dim3(64), 0, c->stream, c->d_efpd, c->d_scratch, c->d_thr, c->d_out, 0);
        else if (N > 512) hipLaunchKernelGGL((acx::sw_kernel<16>), dim3(1, 1), dim3(64), 0, c->stream, c->d_efpd, c->d_scratch, c->d_thr, c->d_out, 0);
        else hipLaunchKernelGGL((acx::sw_kernel<8>), dim3(1, 1), dim3(64), 0, c->stream, c->d_efpd, c->d_scratch, c->d_thr, c->d_out, 0);
        ACX_HIP(c, hipGetLastError());
        ACX_HIP(c, hipMemcpyAsync(sc, c->d_out, sizeof(float) * 4, hipMemcpyDeviceToHost, c->stream));
        ACX_HIP(c, hipStreamSynchronize(c->stream));
        *score = sc[0];
        return ACX_OK;
    });
}

int acx_sw_bits_binary(acx_ctx *c, const uint8_t *B, int32_t M, int32_t N, float *score)
{
    if (!c) return ACX_ERR_INVALID;
    acx::EfPair d;
    std::vector<uint32_t> W;
    float sc[4] = {0, 0, 0, 0};
    return guarded(c, [&]() -> int {
        if (!B || !score || M < 1 || N < 1) return fail(c, ACX_ERR_INVALID, "sw_bits_binary: bad argument");
        if (M > acx::EF_MAXNB || N > acx::EF_MAXNB) return fail(c, ACX_ERR_INVALID, "sw_bits_binary: more than 1024 rows or columns (the bit kernels hold a row in one wave)");
        int rc;
        if ((rc = stage_ef_bit_plot(c, "", B, M, N, d, W)) != ACX_OK) return rc;
        if ((rc = ensure(c, c->d_out, (size_t)4)) != ACX_OK) return rc;
        if (N > 512) hipLaunchKernelGGL((acx::sw_bits_h16_kernel<16>), dim3(1, 1), dim3(64), 0, c->stream, c->d_efpd, c->d_efbits, c->d_out, 0);
        else hipLaunchKernelGGL((acx::sw_bits_h16_kernel<8>), dim3(1, 1), dim3(64), 0, c->stream, c->d_efpd, c->d_efbits, c->d_out, 0);
        ACX_HIP(c, hipGetLastError());
        ACX_HIP(c, hipMemcpyAsync(sc, c->d_out, sizeof(float) * 4, hipMemcpyDeviceToHost, c->stream));
        ACX_HIP(c, hipStreamSynchronize(c->stream));
        *score = sc[0];
        return ACX_OK;
    });
}

// ---------------------------------------------------------------------------------------
// EarlyFusion: where the Smith-Waterman alignment lies, and its path
// ---------------------------------------------------------------------------------------
static const char *const EF_ALIGN_TOO_LONG = "alignment needs the bit path: at most 1024 blocks";

// opts (acx_ef_align_sections): every section of a pair -- `out` holds max_sections records a pair, n_sections
// their numbers, path_off one entry per record; `who` names the entry point in errors.
static int ef_align_impl(acx_ctx *c, const int32_t *pairs, int64_t K, const acx_ef_params *params, int32_t plane, acx_alignment *out,
                         int64_t *path_off, int32_t *cells, int64_t cap, bool any_length, const acx_section_opts *opts = nullptr,
                         int32_t *n_sections = nullptr, const std::string &who = "ef_align")
{
    if (K < 0 || (K > 0 && (!pairs || !out)) || !params || cap < 0) return fail(c, ACX_ERR_INVALID, who + ": bad argument");
    if ((path_off == nullptr) != (cells == nullptr))
        return fail(c, ACX_ERR_INVALID, who + ": path_off and cells must both be given (the paths) or both be NULL (the records alone)");
    if (plane < 0 || plane > 3) return fail(c, ACX_ERR_INVALID, who + ": plane must be 0..3 (mfccs, ssms, chromas, early), got " + std::to_string(plane));
    const int S = opts ? opts->max_sections : 1;                 // records a pair
    if (path_off) path_off[0] = 0;
    if (K == 0) return ACX_OK;
    // the whole list before the first launch, on the caller's list (the sorted copy below would name a pair by its sorted position)
    int64_t good;                                // (this entry's own rule comes before a later track without blocks)
    int rc = check_ef_pairs(c, pairs, K, &good);
    if (rc != ACX_OK) return rc;
    const acx::EfLengths len{c->h_efoff.data(), c->ef_ntracks};
    int64_t bound = 0;                           // no path has more cells than its matrix's shorter side
    for (int64_t k = 0; k < good; ++k) {
        const int64_t M = len.blocks(pairs[2 * k]), N = len.blocks(pairs[2 * k + 1]);
        if (!any_length && (M > acx::EF_MAXNB || N > acx::EF_MAXNB))
            return fail(c, ACX_ERR_UNSUPPORTED, who + ": " + EF_ALIGN_TOO_LONG + " (pair " + std::to_string(k) + ": " + std::to_string(M) + " x " + std::to_string(N) + ")");
        bound += opts ? path_cells_bound((int)M, (int)N, S) : std::min(M, N);
    }
    if (good < K) return ef_short_pair(c, good);
    if (path_off && cap < bound)
        return fail(c, ACX_ERR_INVALID, who + ": cap " + std::to_string(cap) + " is too small: " + std::to_string(bound) + " cells required (the sum of " +
                                            (opts ? "min(M, max_sections * min(M, N))" : "min(M, N)") + " over the list)");
    // the list runs in run order, as acx_earlyfusion_pairs runs it; results go back in the caller's order
    std::vector<int64_t> order;
    std::vector<int32_t> sp;
    const bool sorted = acx::ef_run_order(pairs, K, order, sp);
    auto callers = [&](int64_t k) { return sorted ? k : order[(size_t)k]; };      // pair k of the run -> the caller's pair
    std::vector<float> so((size_t)4 * K);
    std::vector<acx_alignment> sal((size_t)K * S);
    std::vector<int32_t> sn(opts ? (size_t)K : 0);
    std::vector<std::vector<int32_t>> paths(path_off ? (size_t)K * S : 0);
    const EfAlign aln{plane, sal.data(), path_off ? &paths : nullptr, any_length, opts, sn.data()};
    rc = run_ef(c, sorted ? pairs : sp.data(), K, *params, so.data(), nullptr, nullptr, 0, 0, nullptr, &aln);
    if (rc != ACX_OK) return rc;
    for (int64_t k = 0; k < K; ++k) {
        std::copy(sal.begin() + k * S, sal.begin() + (k + 1) * S, out + callers(k) * S);
        if (opts) n_sections[callers(k)] = sn[(size_t)k];
    }
    if (path_off) {
        std::vector<int64_t> where((size_t)K);                       // caller's pair -> its position in the run
        for (int64_t k = 0; k < K; ++k) where[(size_t)callers(k)] = k;
        int64_t n = 0;
        for (int64_t t = 0; t < K * S; ++t) {                        // record t of the caller's list: section t % S of its pair t / S
            const std::vector<int32_t> &pk = paths[(size_t)(where[(size_t)(t / S)] * S + t % S)];
            if (!pk.empty()) memcpy(cells + 2 * n, pk.data(), sizeof(int32_t) * pk.size());
            n += (int64_t)pk.size() / 2;
            path_off[t + 1] = n;
        }
    }
    return ACX_OK;
}

int acx_ef_align(acx_ctx *c, const int32_t *pairs, int64_t K, const acx_ef_params *params, int32_t plane, acx_alignment *out,
                 int64_t *path_off, int32_t *cells, int64_t cap)
{
    if (!c) return ACX_ERR_INVALID;
    return guarded(c, [&] { return ef_align_impl(c, pairs, K, params, plane, out, path_off, cells, cap, false); });
}

// The same for tracks of any length: a list without a track of more than 1024 blocks runs exactly as above; any
// other takes the float path, and ef_align_long_kernel aligns ALL its pairs.
int acx_ef_align_long(acx_ctx *c, const int32_t *pairs, int64_t K, const acx_ef_params *params, int32_t plane, acx_alignment *out,
                      int64_t *path_off, int32_t *cells, int64_t cap)
{
    if (!c) return ACX_ERR_INVALID;
    return guarded(c, [&] { return ef_align_impl(c, pairs, K, params, plane, out, path_off, cells, cap, true); });
}

// ef_align_kernel (acx_sw_align_binary: the plot as bit words, at most 1024 rows and columns) or ef_align_long_kernel
// (acx_sw_align_long_binary, `any_size`: the plot as acx_sw_binary sets it up for sw_long_kernel) alone on a caller's plot: one job, no
// profile entry; `who` names the entry point in errors.
static int sw_align_plot(acx_ctx *c, const std::string &who, bool any_size, const uint8_t *B, int32_t M, int32_t N, acx_alignment *out,
                         int32_t *cells, int64_t cap, int64_t *n_cells)
{
    acx::EfPair d;
    std::vector<acx::EfAlignJob> jobs(1);
    std::vector<uint32_t> W;
    std::vector<float> Cm;
    std::vector<int32_t> res;
    return guarded(c, [&]() -> int {
        if (!B || !out || M < 1 || N < 1 || cap < 0 || (cells != nullptr) != (n_cells != nullptr)) return fail(c, ACX_ERR_INVALID, who + ": bad argument");
        if (!any_size && (M > acx::EF_MAXNB || N > acx::EF_MAXNB)) return fail(c, ACX_ERR_UNSUPPORTED, who + ": " + EF_ALIGN_TOO_LONG);
        if (cells && cap < std::min(M, N))
            return fail(c, ACX_ERR_INVALID, who + ": cap " + std::to_string(cap) + " is too small: " + std::to_string(std::min(M, N)) +
                                                " cells required (min(M, N))");
        if (n_cells) *n_cells = 0;
        int rc = any_size ? stage_ef_float_plot(c, who, B, M, N, d, Cm) : stage_ef_bit_plot(c, who, B, M, N, d, W);
        if (rc != ACX_OK) return rc;
        jobs[0].pair = 0; jobs[0].max_cells = std::min(M, N); jobs[0].dir_off = 0; jobs[0].cell_off = 0;
        const int64_t words = any_size ? acx::ef_align_long_dir_words(M, N) : acx::ef_align_dir_words(M, d.pitchC);
        if ((rc = run_ef_align_jobs(c, jobs, words, {any_size, 0, nullptr, cells != nullptr, -1}, res)) != ACX_OK) return rc;
        std::vector<int32_t> path;
        if ((rc = decode_ef_alignment(c, who, "", res.data(), cells ? res.data() + acx::EFA_REC : nullptr, jobs[0].max_cells, nullptr, *out, cells ? &path : nullptr)) != ACX_OK)
            return rc;
        if (cells) {
            if (!path.empty()) memcpy(cells, path.data(), sizeof(int32_t) * path.size());
            *n_cells = (int64_t)path.size() / 2;
        }
        return ACX_OK;
    });
}

int acx_sw_align_binary(acx_ctx *c, const uint8_t *B, int32_t M, int32_t N, acx_alignment *out, int32_t *cells, int64_t cap, int64_t *n_cells)
{
    if (!c) return ACX_ERR_INVALID;
    return sw_align_plot(c, "sw_align_binary", false, B, M, N, out, cells, cap, n_cells);
}

int acx_sw_align_long_binary(acx_ctx *c, const uint8_t *B, int32_t M, int32_t N, acx_alignment *out, int32_t *cells, int64_t cap, int64_t *n_cells)
{
    if (!c) return ACX_ERR_INVALID;
    return sw_align_plot(c, "sw_align_long_binary", true, B, M, N, out, cells, cap, n_cells);
}

// ---- every section of a pair ----
int acx_ef_align_sections(acx_ctx *c, const int32_t *pairs, int64_t K, const acx_ef_params *params, int32_t plane, const acx_section_opts *opts,
                          acx_alignment *out, int32_t *n_sections, int64_t *path_off, int32_t *cells, int64_t cap)
{
    if (!c) return ACX_ERR_INVALID;
    const std::string who = "ef_align_sections";
    return guarded(c, [&]() -> int {
        if (!opts || (K > 0 && !n_sections)) return fail(c, ACX_ERR_INVALID, who + ": bad argument");
        int rc = check_section_opts(c, who, *opts);
        if (rc != ACX_OK) return rc;
        return ef_align_impl(c, pairs, K, params, plane, out, path_off, cells, cells ? cap : 0, false, opts, n_sections, who);
    });
}

// ef_sections_kernel alone on a caller's plot, staged as acx_sw_align_binary stages it: one job.
int acx_sw_sections_binary(acx_ctx *c, const uint8_t *B, int32_t M, int32_t N, const acx_section_opts *opts, acx_alignment *out,
                           int32_t *n_sections, int64_t *path_off, int32_t *cells, int64_t cap)
{
    if (!c) return ACX_ERR_INVALID;
    const std::string who = "sw_sections_binary";
    acx::EfPair d;
    std::vector<acx::EfAlignJob> jobs(1);
    std::vector<uint32_t> W;
    std::vector<int32_t> res;
    return guarded(c, [&]() -> int {
        if (!B || !opts || !out || !n_sections || M < 1 || N < 1 || (path_off == nullptr) != (cells == nullptr) || (cells && cap < 0))
            return fail(c, ACX_ERR_INVALID, who + ": bad argument");
        int rc = check_section_opts(c, who, *opts);
        if (rc != ACX_OK) return rc;
        const int S = opts->max_sections;
        if (M > acx::EF_MAXNB || N > acx::EF_MAXNB) return fail(c, ACX_ERR_UNSUPPORTED, who + ": " + EF_ALIGN_TOO_LONG);
        const int64_t room = acx::ef_sections_room(M, N, S);
        if (cells && cap < room)
            return fail(c, ACX_ERR_INVALID, who + ": cap " + std::to_string(cap) + " is too small: " + std::to_string(room) +
                                                " cells required (min(M, max_sections * min(M, N)))");
        if (path_off) path_off[0] = 0;
        if ((rc = stage_ef_bit_plot(c, who, B, M, N, d, W)) != ACX_OK) return rc;
        jobs[0].pair = 0; jobs[0].max_cells = (int)room; jobs[0].dir_off = 0; jobs[0].cell_off = 0;
        const size_t nrec = ef_align_nrec(1, S);
        if ((rc = run_ef_align_jobs(c, jobs, acx::ef_align_dir_words(M, d.pitchC), {false, 0, opts, cells != nullptr, (int64_t)M * N}, res)) != ACX_OK) return rc;
        drain_profile(c);
        std::vector<std::vector<int32_t>> paths(cells ? (size_t)S : 0);
        if ((rc = decode_ef_sections(c, who, "", S, res[0], res.data() + 1, cells ? res.data() + nrec : nullptr, room, std::min(M, N), nullptr,
                                     opts->min_score, out, *n_sections, cells ? paths.data() : nullptr)) != ACX_OK)
            return rc;
        if (cells) pack_paths(paths, path_off, cells);
        return ACX_OK;
    });
}

// ---------------------------------------------------------------------------------------
// FTM2D (ftm2d.py): shingles of raw chroma + beat onsets built on the device, pair scores
// ---------------------------------------------------------------------------------------
void acx_ftm2d_default_params(acx_ftm2d_params *p)
{
    if (!p) return;
    p->pwr = 1.96;      // FTM2D ctor, ftm2d.py:23
    p->c = 5.0;
    p->win = 75;
    p->reserved = 0;
}

static int ftm2d_check_params(acx_ctx *c, const char *who, const acx_ftm2d_params *p)
{
    if (!p) return fail(c, ACX_ERR_INVALID, std::string(who) + ": params must not be NULL");
    if (p->win < 1 || p->win > acx::FTM_MAXWIN)
        return fail(c, ACX_ERR_INVALID, std::string(who) + ": WIN must be in 1..256 on the device (got " + std::to_string(p->win) + ")");
    if (!std::isfinite(p->pwr) || !std::isfinite(p->c)) return fail(c, ACX_ERR_INVALID, std::string(who) + ": PWR and C must be finite");
    return ACX_OK;
}

static void ftm2d_free_pool(acx_ctx *c)
{
    (void)c->d_ftm.reset();
    c->ftm_n = c->ftm_dim = 0;
    c->ftm_open = 0;
    c->ftm_filled.clear();
}

// Host copies of one track's intermediates (acx_ftm2d_debug_track); any may be NULL.
struct FtmDebug { float *synced; double *pwr, *logwin, *median; };

// Shingles of tracks [0, nt) (chroma rows coff[t] .. coff[t + 1], onsets ooff[t] .. ooff[t + 1]) into d_out, a DEVICE
// (nt, 12 WIN) f64 array.  Every track is checked before the first launch (negative onset, fewer beats than WIN, a
// window matrix beyond the scratch limit); `track_base` only names tracks in messages.  Then sub-batches of whole
// tracks whose window matrices fit the scratch limit (and whose chroma fits RAW_SLICE_FLOATS) run F1 .. F5.
static int ftm2d_build(acx_ctx *c, const char *who, const float *chroma, const int64_t *coff, const int64_t *onsets,
                       const int64_t *ooff, int32_t nt, int32_t track_base, const acx_ftm2d_params &p, double *d_out,
                       const FtmDebug *dbg)
{
    const int win = p.win, D = 12 * win;
    const int64_t lim = std::min<int64_t>(scratch_limit_bytes(c), (int64_t)4 << 30);     // window matrices per sub-batch (bytes)
    // librosa.util.sync(X, onsets, pad=True): boundaries unique(clip(onsets, 0, T) + {0, T}), librosa.util.fix_frames
    std::vector<int64_t> nbeat((size_t)nt), bnd;
    std::vector<std::vector<int64_t>> tb((size_t)nt);
    for (int t = 0; t < nt; ++t) {
        if (coff[t + 1] < coff[t] || ooff[t + 1] < ooff[t]) return fail(c, ACX_ERR_INVALID, std::string(who) + ": offsets must be non-decreasing");
        const int64_t T = coff[t + 1] - coff[t];
        std::vector<int64_t> &b = tb[t];
        b.reserve((size_t)(ooff[t + 1] - ooff[t]) + 2);
        b.push_back(0);
        b.push_back(T);
        for (int64_t k = ooff[t]; k < ooff[t + 1]; ++k) {
            if (onsets[k] < 0)
                return fail(c, ACX_ERR_INVALID, std::string(who) + ": track " + std::to_string(track_base + t) + " has a negative onset (" +
                            std::to_string(onsets[k]) + "); librosa.util.fix_frames raises there");
            b.push_back(std::min(onsets[k], T));
        }
        std::sort(b.begin(), b.end());
        b.erase(std::unique(b.begin(), b.end()), b.end());
        nbeat[t] = (int64_t)b.size() - 1;
        if (nbeat[t] < win)
            return fail(c, ACX_ERR_INVALID, std::string(who) + ": track " + std::to_string(track_base + t) + " has " + std::to_string(nbeat[t]) +
                        " beats, fewer than WIN = " + std::to_string(win) + " (btchroma_to_fftmat returns None there)");
        if ((nbeat[t] - win + 1) * D * (int64_t)sizeof(double) > lim)
            return fail(c, ACX_ERR_NOMEM, std::string(who) + ": the window matrix of track " + std::to_string(track_base + t) + " does not fit the scratch limit");
    }
    // twiddles exp(-2 pi i m / n), n = 12 and WIN
    std::vector<double> tw12(24), twW(2 * (size_t)win);
    for (int m = 0; m < 12; ++m) { tw12[2 * m] = std::cos(2.0 * M_PI * m / 12.0); tw12[2 * m + 1] = -std::sin(2.0 * M_PI * m / 12.0); }
    for (int m = 0; m < win; ++m) { twW[2 * m] = std::cos(2.0 * M_PI * m / win); twW[2 * m + 1] = -std::sin(2.0 * M_PI * m / win); }
    // windows per workgroup of ftm2d_window_kernel: as many (<= 8) as LDS holds
    auto lds_bytes = [&](int nw) { return sizeof(double) * (size_t)(2 * 7 * (nw + win - 1) + 2 * win + nw * 7 * win + nw); };
    int nw = acx::FTM_NW;
    while (nw > 1 && lds_bytes(nw) > (size_t)acx::FTM_LDS) --nw;
    DeviceBuffer<double> d_tw;
    ACX_HIP(c, d_tw.grow(24 + 2 * (size_t)win));
    ACX_HIP(c, hipMemcpy(d_tw, tw12.data(), sizeof(double) * 24, hipMemcpyHostToDevice));
    ACX_HIP(c, hipMemcpy(d_tw + 24, twW.data(), sizeof(double) * 2 * win, hipMemcpyHostToDevice));
    DeviceBuffer<float> d_ch, d_sync;                // staging and intermediates of one slice: grown as needed, reused by the next
    DeviceBuffer<int64_t> d_coff, d_bnd, d_boff, d_woff;
    DeviceBuffer<double> d_pwr, d_G, d_lw, d_med;
    DeviceBuffer<acx::FtmBlock> d_blk;
    // a slice: its window matrices within `lim`, its chroma within the staging budget
    std::vector<int64_t> wbytes((size_t)nt + 1, 0);
    for (int t = 0; t < nt; ++t) wbytes[t + 1] = wbytes[t] + (nbeat[t] - win + 1) * D * (int64_t)sizeof(double);
    const int64_t budget = raw_slice_bytes(c);
    auto fits = [&](int t0, int t1) { return wbytes[t1] - wbytes[t0] <= lim && (coff[t1] - coff[t0]) * 12 * (int64_t)sizeof(float) <= budget; };
    return for_track_slices(nt, 65535, fits, [&](int t0, int t1) -> int {
        const int n = t1 - t0;
        const int64_t rows = coff[t1] - coff[t0];
        std::vector<int64_t> lc(n + 1), lb(n + 1), lwo(n + 1), lbnd;
        std::vector<acx::FtmBlock> blk;
        lc[0] = lb[0] = lwo[0] = 0;
        for (int t = 0; t < n; ++t) {
            lc[t + 1] = coff[t0 + t + 1] - coff[t0];
            lb[t + 1] = lb[t] + nbeat[t0 + t];
            const int64_t nwin = nbeat[t0 + t] - win + 1;
            lwo[t + 1] = lwo[t] + nwin;
            for (int64_t b : tb[t0 + t]) lbnd.push_back(lc[t] + b);
            for (int64_t w = 0; w < nwin; w += nw) blk.push_back(acx::FtmBlock{t, (int32_t)w});
        }
        const int64_t nb = lb[n], nwt = lwo[n];
        ACX_HIP(c, d_ch.grow((size_t)std::max<int64_t>(1, rows) * 12));
        ACX_HIP(c, d_coff.grow((size_t)n + 1));
        ACX_HIP(c, d_bnd.grow(lbnd.size()));
        ACX_HIP(c, d_boff.grow((size_t)n + 1));
        ACX_HIP(c, d_woff.grow((size_t)n + 1));
        ACX_HIP(c, d_sync.grow((size_t)nb * 12));
        ACX_HIP(c, d_pwr.grow((size_t)nb * 12));
        ACX_HIP(c, d_G.grow((size_t)nb * 14));
        ACX_HIP(c, d_lw.grow((size_t)nwt * D));
        ACX_HIP(c, d_med.grow((size_t)n * D));
        ACX_HIP(c, d_blk.grow(blk.size()));
        ACX_HIP(c, hipMemcpyAsync(d_ch, chroma + coff[t0] * 12, sizeof(float) * rows * 12, hipMemcpyHostToDevice, c->stream));
        ACX_HIP(c, hipMemcpyAsync(d_coff, lc.data(), sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, c->stream));
        ACX_HIP(c, hipMemcpyAsync(d_bnd, lbnd.data(), sizeof(int64_t) * lbnd.size(), hipMemcpyHostToDevice, c->stream));
        ACX_HIP(c, hipMemcpyAsync(d_boff, lb.data(), sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, c->stream));
        ACX_HIP(c, hipMemcpyAsync(d_woff, lwo.data(), sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, c->stream));
        ACX_HIP(c, hipMemcpyAsync(d_blk, blk.data(), sizeof(acx::FtmBlock) * blk.size(), hipMemcpyHostToDevice, c->stream));
        {   // (the host buffers above are pageable: the copies are staged before the calls return)
            const int rcs = scan_nonfinite(c, who, "chroma", d_ch.get(), rows * 12, 12, 0, d_coff.get(), n, false, track_base + t0);
            if (rcs != ACX_OK) return rcs;
        }
        hipLaunchKernelGGL(acx::ftm2d_sync_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, c->stream, d_ch, d_bnd, d_boff, n, nb, d_sync);
        hipLaunchKernelGGL(acx::ftm2d_beat_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, c->stream, d_sync, nb, p.pwr, d_tw, d_pwr, d_G);
        hipLaunchKernelGGL(acx::ftm2d_window_kernel, dim3((unsigned)blk.size()), dim3(256), lds_bytes(nw), c->stream, d_G, d_boff, d_woff, d_blk,
                           d_tw + 24, win, nw, p.c, d_lw);
        int maxw = 0;
        for (int t = 0; t < n; ++t) maxw = std::max<int>(maxw, (int)(lwo[t + 1] - lwo[t]));
        if (maxw <= 64 * 8)
            hipLaunchKernelGGL((acx::ftm2d_median_kernel<8>), dim3((D + 3) / 4, n), dim3(256), 0, c->stream, d_lw, d_woff, D, d_med);
        else
            hipLaunchKernelGGL((acx::ftm2d_median_kernel<32>), dim3((D + 3) / 4, n), dim3(256), 0, c->stream, d_lw, d_woff, D, d_med);
        hipLaunchKernelGGL(acx::ftm2d_normalize_kernel, dim3(n), dim3(64), 0, c->stream, d_med, D, d_out + (int64_t)t0 * D);
        ACX_HIP(c, hipGetLastError());
        if (dbg) {      // one track
            if (dbg->synced) ACX_HIP(c, hipMemcpyAsync(dbg->synced, d_sync, sizeof(float) * nb * 12, hipMemcpyDeviceToHost, c->stream));
            if (dbg->pwr) ACX_HIP(c, hipMemcpyAsync(dbg->pwr, d_pwr, sizeof(double) * nb * 12, hipMemcpyDeviceToHost, c->stream));
            if (dbg->median) ACX_HIP(c, hipMemcpyAsync(dbg->median, d_med, sizeof(double) * D, hipMemcpyDeviceToHost, c->stream));
            if (dbg->logwin) {      // (D, nwin) on the device -> (nwin, D) like btchroma_to_fftmat(...).T
                std::vector<double> h((size_t)nwt * D);
                ACX_HIP(c, hipMemcpyAsync(h.data(), d_lw, sizeof(double) * h.size(), hipMemcpyDeviceToHost, c->stream));
                ACX_HIP(c, hipStreamSynchronize(c->stream));
                for (int64_t w = 0; w < nwt; ++w)
                    for (int d = 0; d < D; ++d) dbg->logwin[w * D + d] = h[(size_t)d * nwt + w];
            }
        }
        ACX_HIP(c, hipStreamSynchronize(c->stream));
        return ACX_OK;
    });
}

int acx_ftm2d_pool_begin(acx_ctx *c, int32_t n_tracks, const acx_ftm2d_params *params)
{
    if (!c) return ACX_ERR_INVALID;
    int rc = ftm2d_check_params(c, "ftm2d_pool_begin", params);
    if (rc != ACX_OK) return rc;
    if (n_tracks < 1) return fail(c, ACX_ERR_INVALID, "ftm2d_pool_begin: n_tracks must be >= 1");
    ACX_HIP(c, hipSetDevice(c->device));
    ftm2d_free_pool(c);
    const int D = 12 * params->win;
    const hipError_t e = c->d_ftm.grow((size_t)n_tracks * D);
    if (e != hipSuccess) return fail(c, ACX_ERR_NOMEM, std::string("ftm2d_pool_begin: ") + hipGetErrorString(e));
    c->ftm_n = n_tracks;
    c->ftm_dim = D;
    c->ftm_open = n_tracks;
    c->ftm_filled.assign((size_t)n_tracks, 0);
    c->ftm_params = *params;
    return ACX_OK;
}

int acx_ftm2d_pool_tracks(acx_ctx *c, int32_t first_track, int32_t count, const float *chroma, const int64_t *chroma_offsets,
                          const int64_t *onsets, const int64_t *onset_offsets)
{
    if (!c) return ACX_ERR_INVALID;
    if (!c->ftm_open) return fail(c, ACX_ERR_STATE, "ftm2d_pool_tracks: no pool is open (acx_ftm2d_pool_begin)");
    if (!chroma || !chroma_offsets || !onsets || !onset_offsets || count < 1 || first_track < 0 || first_track > c->ftm_n - count)
        return fail(c, ACX_ERR_INVALID, "ftm2d_pool_tracks: bad argument (tracks must lie in the open pool)");
    ACX_HIP(c, hipSetDevice(c->device));
    c->nf_zeroed = 0;
    const int rc = ftm2d_build(c, "ftm2d_pool_tracks", chroma, chroma_offsets, onsets, onset_offsets, count, first_track, c->ftm_params,
                               c->d_ftm + (int64_t)first_track * c->ftm_dim, nullptr);
    if (rc != ACX_OK) return rc;
    for (int t = 0; t < count; ++t) c->ftm_filled[(size_t)first_track + t] = 1;
    return ACX_OK;
}

int acx_ftm2d_pool_end(acx_ctx *c)
{
    if (!c) return ACX_ERR_INVALID;
    if (!c->ftm_open) return fail(c, ACX_ERR_STATE, "ftm2d_pool_end: no pool is open (acx_ftm2d_pool_begin)");
    for (int t = 0; t < c->ftm_n; ++t)
        if (!c->ftm_filled[t]) return fail(c, ACX_ERR_STATE, "ftm2d_pool_end: track " + std::to_string(t) + " was never handed over (acx_ftm2d_pool_tracks)");
    c->ftm_open = 0;
    c->ftm_filled.clear();
    return ACX_OK;
}

int acx_ftm2d_upload_shingles(acx_ctx *c, const double *shingles, int32_t n_tracks, int32_t dim)
{
    if (!c) return ACX_ERR_INVALID;
    if (!shingles || n_tracks < 1 || dim < 1) return fail(c, ACX_ERR_INVALID, "ftm2d_upload_shingles: bad argument");
    ACX_HIP(c, hipSetDevice(c->device));
    ftm2d_free_pool(c);
    const size_t n = (size_t)n_tracks * dim;
    const hipError_t e = c->d_ftm.grow(n);
    if (e != hipSuccess) return fail(c, ACX_ERR_NOMEM, std::string("ftm2d_upload_shingles: ") + hipGetErrorString(e));
    ACX_HIP(c, hipMemcpy(c->d_ftm, shingles, sizeof(double) * n, hipMemcpyHostToDevice));
    c->ftm_n = n_tracks;
    c->ftm_dim = dim;
    return ACX_OK;
}

int acx_ftm2d_download_shingles(acx_ctx *c, double *shingles, int64_t capacity)
{
    if (!c) return ACX_ERR_INVALID;
    if (!c->d_ftm || c->ftm_open) return fail(c, ACX_ERR_STATE, "ftm2d_download_shingles: no shingle pool (acx_ftm2d_pool_* or acx_ftm2d_upload_shingles)");
    const int64_t need = (int64_t)c->ftm_n * c->ftm_dim;
    if (!shingles || capacity < need) return fail(c, ACX_ERR_INVALID, "ftm2d_download_shingles: buffer too small");
    ACX_HIP(c, hipSetDevice(c->device));
    ACX_HIP(c, hipMemcpy(shingles, c->d_ftm, sizeof(double) * need, hipMemcpyDeviceToHost));
    return ACX_OK;
}

int acx_ftm2d_debug_track(acx_ctx *c, const float *chroma, int64_t n_frames, const int64_t *onsets, int64_t n_onsets,
                          const acx_ftm2d_params *params, float *synced, double *pwr, double *logwin, double *median,
                          double *shingle, int64_t *dims)
{
    if (!c) return ACX_ERR_INVALID;
    int rc = ftm2d_check_params(c, "ftm2d_debug_track", params);
    if (rc != ACX_OK) return rc;
    if (!chroma || !onsets || n_frames < 0 || n_onsets < 0 || !dims) return fail(c, ACX_ERR_INVALID, "ftm2d_debug_track: bad argument");
    const int64_t coff[2] = {0, n_frames}, ooff[2] = {0, n_onsets};
    {   // the shape first (the same boundaries ftm2d_build computes)
        std::vector<int64_t> b = {0, n_frames};
        for (int64_t k = 0; k < n_onsets; ++k) b.push_back(std::min(std::max<int64_t>(onsets[k], 0), n_frames));
        std::sort(b.begin(), b.end());
        b.erase(std::unique(b.begin(), b.end()), b.end());
        const int64_t nb = (int64_t)b.size() - 1;
        dims[0] = nb;
        dims[1] = std::max<int64_t>(0, nb - params->win + 1);
        dims[2] = 12 * (int64_t)params->win;
    }
    if (!synced && !pwr && !logwin && !median && !shingle) return ACX_OK;
    ACX_HIP(c, hipSetDevice(c->device));
    c->nf_zeroed = 0;
    DeviceBuffer<double> d_s;
    ACX_HIP(c, d_s.grow((size_t)12 * params->win));
    FtmDebug dbg{synced, pwr, logwin, median};
    rc = ftm2d_build(c, "ftm2d_debug_track", chroma, coff, onsets, ooff, 1, 0, *params, d_s, &dbg);
    if (rc == ACX_OK && shingle) {
        const hipError_t e = hipMemcpy(shingle, d_s, sizeof(double) * 12 * params->win, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(c, ACX_ERR_HIP, std::string("ftm2d_debug_track: ") + hipGetErrorString(e));
    }
    return rc;
}

int acx_ftm2d_pairs(acx_ctx *c, const int32_t *pairs, int64_t K, float *out)
{
    if (!c) return ACX_ERR_INVALID;
    if (K < 0 || (K > 0 && (!pairs || !out))) return fail(c, ACX_ERR_INVALID, "ftm2d_pairs: bad argument");
    if (!c->d_ftm || c->ftm_open) return fail(c, ACX_ERR_STATE, "ftm2d_pairs: no shingle pool (acx_ftm2d_pool_* or acx_ftm2d_upload_shingles)");
    for (int64_t k = 0; k < K; ++k)     // the whole list before the first launch
        if (pairs[2 * k] < 0 || pairs[2 * k + 1] < 0 || pairs[2 * k] >= c->ftm_n || pairs[2 * k + 1] >= c->ftm_n)
            return fail(c, ACX_ERR_INVALID, "ftm2d_pairs: track index out of range in pair " + std::to_string(k));
    if (K == 0) return ACX_OK;
    ACX_HIP(c, hipSetDevice(c->device));
    const int64_t CH = (int64_t)1 << 22;
    int rc;
    if ((rc = ensure(c, c->d_pairs, (size_t)2 * std::min(K, CH))) != ACX_OK) return rc;
    if ((rc = ensure(c, c->d_out, (size_t)std::min(K, CH))) != ACX_OK) return rc;
    for (int64_t k0 = 0; k0 < K; k0 += CH) {
        const int64_t n = std::min(CH, K - k0);
        ACX_HIP(c, hipMemcpyAsync(c->d_pairs, pairs + 2 * k0, sizeof(int32_t) * 2 * n, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(acx::ftm2d_pairs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->d_ftm, c->ftm_dim,
                           c->d_pairs, n, c->d_out);
        ACX_HIP(c, hipGetLastError());
        ACX_HIP(c, hipMemcpyAsync(out + k0, c->d_out, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
        ACX_HIP(c, hipStreamSynchronize(c->stream));
    }
    return ACX_OK;
}

// ---------------------------------------------------------------------------------------
// Ranking of finished score rows (rank_kernels.hpp): evaluation positions and top-k lists
// ---------------------------------------------------------------------------------------
static const int64_t RANK_SLICE_BYTES = (int64_t)64 << 20;       // a staging piece of whole rows (two are in flight)

// What both calls check of their common arguments, before anything is allocated or launched.
static int rank_check_common(acx_ctx *c, const char *who, const float *scores, int64_t ld, int32_t n, int32_t n_rows, const int32_t *self,
                             const int32_t *posn)
{
    const std::string w(who);
    if (n < 1) return fail(c, ACX_ERR_INVALID, w + ": n must be >= 1 (got " + std::to_string(n) + ")");
    if (n_rows < 0) return fail(c, ACX_ERR_INVALID, w + ": n_rows must be >= 0 (got " + std::to_string(n_rows) + ")");
    if (ld < n) return fail(c, ACX_ERR_INVALID, w + ": ld = " + std::to_string(ld) + " is smaller than n = " + std::to_string(n));
    if (n_rows > 0 && (!scores || !self)) return fail(c, ACX_ERR_INVALID, w + ": scores and self must not be NULL");
    for (int32_t r = 0; r < n_rows; ++r)
        if (self[r] < 0 || self[r] >= n)
            return fail(c, ACX_ERR_INVALID, w + ": self[" + std::to_string(r) + "] = " + std::to_string(self[r]) + " is not a column in [0, " + std::to_string(n) + ")");
    if (posn)
        for (int32_t i = 0; i < n; ++i)
            if (posn[i] < 0) return fail(c, ACX_ERR_INVALID, w + ": posn[" + std::to_string(i) + "] = " + std::to_string(posn[i]) + " is negative");
    return ACX_OK;
}

// What the two position calls check of a mate list.  `item`: what a mate is ("column" / "track"); a mate that is row r's
// own (own[r]) is reported as "mates[j] <own_a>r<own_b>".
static int rank_check_mates(acx_ctx *c, const char *who, int32_t n, int32_t n_rows, const int32_t *own, const char *item, const char *own_a,
                            const char *own_b, const int64_t *moff, const int32_t *mates, const int32_t *out_pos, const uint8_t *out_flag)
{
    const std::string w(who);
    if (!moff) return fail(c, ACX_ERR_INVALID, w + ": moff must not be NULL");
    if (moff[0] != 0) return fail(c, ACX_ERR_INVALID, w + ": moff[0] must be 0");
    for (int32_t r = 0; r < n_rows; ++r)
        if (moff[r + 1] < moff[r]) return fail(c, ACX_ERR_INVALID, w + ": moff must be non-decreasing (moff[" + std::to_string(r + 1) + "])");
    if (n_rows > 0 && !out_flag) return fail(c, ACX_ERR_INVALID, w + ": out_flag must not be NULL");
    if (moff[n_rows] > 0 && (!mates || !out_pos)) return fail(c, ACX_ERR_INVALID, w + ": mates and out_pos must not be NULL");
    for (int32_t r = 0; r < n_rows; ++r)
        for (int64_t j = moff[r]; j < moff[r + 1]; ++j) {
            if (mates[j] < 0 || mates[j] >= n)
                return fail(c, ACX_ERR_INVALID, w + ": mates[" + std::to_string(j) + "] = " + std::to_string(mates[j]) + " is not a " + item + " in [0, " + std::to_string(n) + ")");
            if (mates[j] == own[r]) return fail(c, ACX_ERR_INVALID, w + ": mates[" + std::to_string(j) + "] " + own_a + std::to_string(r) + own_b);
        }
    return ACX_OK;
}

// What the two top-k calls check of k and their outputs.
static int rank_check_k(acx_ctx *c, const char *who, int32_t k, int32_t n_rows, const int32_t *out_idx, const float *out_score)
{
    const std::string w(who);
    if (k < 1) return fail(c, ACX_ERR_INVALID, w + ": k must be >= 1 (got " + std::to_string(k) + ")");
    if (k > acx::RANK_KMAX) return fail(c, ACX_ERR_UNSUPPORTED, w + ": k = " + std::to_string(k) + " is over the limit of " + std::to_string(acx::RANK_KMAX));
    if (n_rows > 0 && (!out_idx || !out_score)) return fail(c, ACX_ERR_INVALID, w + ": out_idx and out_score must not be NULL");
    return ACX_OK;
}

extern "C++" {
// One device block of `total` bytes for the length of a call: body(d_mem) issues the call's work and returns an ACX code;
// the device is done with the block when it is freed.
template <typename F>
static int with_device_block(acx_ctx *c, const char *who, size_t total, F body)
{
    DeviceBuffer<char> d_mem;
    const hipError_t e = d_mem.grow(total);
    if (e != hipSuccess) return fail(c, ACX_ERR_NOMEM, std::string(who) + ": " + hipGetErrorString(e));
    const int rc = guarded(c, [&] { return body(d_mem.get()); });
    if (rc == ACX_OK) drain_profile(c);
    return rc;
}
}  // extern "C++"

// One launch of a kernel template <bool IN_LDS> of rank_kernels.hpp / query_kernels.hpp (256 threads) on c->stream
#define ACX_LAUNCH_IN_LDS(KERNEL_, in_lds_, grid_, lds_, ...)                                                                        \
    do {                                                                                                                             \
        if (in_lds_) hipLaunchKernelGGL((acx::KERNEL_<true>), grid_, dim3(acx::RANK_THREADS), lds_, c->stream, __VA_ARGS__);         \
        else hipLaunchKernelGGL((acx::KERNEL_<false>), grid_, dim3(acx::RANK_THREADS), lds_, c->stream, __VA_ARGS__);                \
    } while (0)

// Rows per staging piece: whole rows, RANK_SLICE_BYTES at most, and everything the call holds on the device (two pieces,
// `per_row_out` bytes of results per row, `fixed` bytes of tables) within the scratch limit.
static int rank_piece_rows(acx_ctx *c, const char *who, int32_t n, int32_t n_rows, int64_t per_row_out, int64_t fixed, int32_t *rows)
{
    const int64_t row_bytes = (int64_t)round_up(n, 4) * 4;
    const int64_t lim = scratch_limit_bytes(c) - fixed;
    if (lim < 2 * (row_bytes + per_row_out))
        return fail(c, ACX_ERR_NOMEM, std::string(who) + ": two rows of " + std::to_string(n) + " scores and their results do not fit the scratch limit");
    const int64_t pr = std::min<int64_t>(RANK_SLICE_BYTES / row_bytes, lim / (2 * (row_bytes + per_row_out)));
    *rows = (int32_t)std::max<int64_t>(1, std::min<int64_t>(pr, n_rows));
    return ACX_OK;
}

// Stages the slab to the device piece by piece through the two pinned slots and calls run(d_rows, ldd, r0, nr) for every
// piece (run launches on c->stream and returns an ACX code).  The host packs piece p + 1 while piece p is copied and ranked.
extern "C++" {
template <typename F>
static int rank_for_pieces(acx_ctx *c, const float *scores, int64_t ld, int32_t n, int32_t n_rows, int32_t piece, F run)
{
    const int64_t ldd = round_up(n, 4);
    int rc;
    for (int e = 0; e < 2; ++e) {
        const size_t need = (size_t)ldd * piece;
        if (c->rank_h[e].grow(need) != hipSuccess)
            return fail(c, ACX_ERR_NOMEM, "rank: cannot allocate a pinned staging slot of " + std::to_string(need * sizeof(float)) + " bytes");
        if ((rc = ensure(c, c->rank_d[e], need)) != ACX_OK) return rc;
        if (!c->rank_ev[e]) ACX_HIP(c, hipEventCreateWithFlags(&c->rank_ev[e], hipEventDisableTiming));
        if (n_rows <= piece) break;                                        // one piece: one slot
    }
    int p = 0;
    for (int32_t r0 = 0; r0 < n_rows; r0 += piece, ++p) {
        const int32_t nr = std::min(piece, n_rows - r0);
        const int e = p & 1;
        if (p >= 2) ACX_HIP(c, hipEventSynchronize(c->rank_ev[e]));        // the slot's previous piece is done with it
        for (int32_t r = 0; r < nr; ++r) memcpy(c->rank_h[e] + (size_t)r * ldd, scores + (size_t)(r0 + r) * ld, sizeof(float) * (size_t)n);
        ACX_HIP(c, hipMemcpyAsync(c->rank_d[e], c->rank_h[e], sizeof(float) * (size_t)ldd * nr, hipMemcpyHostToDevice, c->stream));
        if ((rc = run(c->rank_d[e], ldd, r0, nr)) != ACX_OK) return rc;
        ACX_HIP(c, hipEventRecord(c->rank_ev[e], c->stream));
    }
    ACX_HIP(c, hipStreamSynchronize(c->stream));
    return ACX_OK;
}
}  // extern "C++"

static int rank_lds_attr(acx_ctx *c)
{
    if (c->rank_attr) return ACX_OK;
    const int row = 4 * acx::RANK_ROW_LDS;
    ACX_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(acx::rank_columns_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   row + acx::RANK_COUNT_LDS_FIXED));
    ACX_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(acx::topk_rows_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   row + 12 * acx::RANK_KMAX + acx::RANK_SELECT_LDS_FIXED));
    c->rank_attr = true;
    return ACX_OK;
}

int acx_rank_columns(acx_ctx *c, const float *scores, int64_t ld, int32_t n, int32_t n_rows, const int32_t *self, const int32_t *posn,
                     const int64_t *moff, const int32_t *mates, int32_t *out_pos, uint8_t *out_flag)
{
    if (!c) return ACX_ERR_INVALID;
    int rc = rank_check_common(c, "rank_columns", scores, ld, n, n_rows, self, posn);
    if (rc != ACX_OK) return rc;
    if ((rc = rank_check_mates(c, "rank_columns", n, n_rows, self, "column", "is row ", "'s own column (self)", moff, mates, out_pos, out_flag)) != ACX_OK)
        return rc;
    const int64_t M = moff[n_rows];
    if (n_rows == 0) return ACX_OK;
    const int64_t fixed = 8 * (int64_t)(n_rows + 1) + 8 * M + 5 * (int64_t)n_rows + 4 * (int64_t)n;
    int32_t piece = 0;
    if ((rc = rank_piece_rows(c, "rank_columns", n, n_rows, 0, fixed, &piece)) != ACX_OK) return rc;
    ACX_HIP(c, hipSetDevice(c->device));
    if ((rc = rank_lds_attr(c)) != ACX_OK) return rc;
    // the tables of the whole call in one device block: moff | mates | out_pos | self | posn | out_flag
    const size_t o_mates = sizeof(int64_t) * (size_t)(n_rows + 1), o_pos = o_mates + 4 * (size_t)M, o_self = o_pos + 4 * (size_t)M,
                 o_posn = o_self + 4 * (size_t)n_rows, o_flag = o_posn + (posn ? 4 * (size_t)n : 0), total = o_flag + (size_t)n_rows;
    return with_device_block(c, "rank_columns", total, [&](char *d_tab) -> int {
        ACX_HIP(c, hipMemcpyAsync(d_tab, moff, sizeof(int64_t) * (size_t)(n_rows + 1), hipMemcpyHostToDevice, c->stream));
        if (M > 0) ACX_HIP(c, hipMemcpyAsync(d_tab + o_mates, mates, 4 * (size_t)M, hipMemcpyHostToDevice, c->stream));
        ACX_HIP(c, hipMemcpyAsync(d_tab + o_self, self, 4 * (size_t)n_rows, hipMemcpyHostToDevice, c->stream));
        if (posn) ACX_HIP(c, hipMemcpyAsync(d_tab + o_posn, posn, 4 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        const int64_t *d_moff = reinterpret_cast<const int64_t *>(d_tab);
        const int32_t *d_mates = reinterpret_cast<const int32_t *>(d_tab + o_mates), *d_self = reinterpret_cast<const int32_t *>(d_tab + o_self);
        const int32_t *d_posn = posn ? reinterpret_cast<const int32_t *>(d_tab + o_posn) : nullptr;
        int32_t *d_pos = reinterpret_cast<int32_t *>(d_tab + o_pos);
        uint8_t *d_flag = reinterpret_cast<uint8_t *>(d_tab + o_flag);
        const bool in_lds = n <= acx::RANK_ROW_LDS;
        const size_t lds = acx::RANK_COUNT_LDS_FIXED + (in_lds ? 16 * (size_t)((n + 3) / 4) : 0);
        int rcp = rank_for_pieces(c, scores, ld, n, n_rows, piece, [&](const float *d_rows, int64_t ldd, int32_t r0, int32_t nr) -> int {
            ProfScope ps(c, KS_RANK, (int64_t)nr * n);
            ACX_LAUNCH_IN_LDS(rank_columns_kernel, in_lds, dim3((unsigned)nr), lds, d_rows, ldd, (int)n, d_self + r0, d_posn, d_moff + r0, d_mates,
                              (int64_t)0, d_pos, d_flag + r0);
            return ACX_OK;
        });
        if (rcp != ACX_OK) return rcp;
        ACX_LAUNCHES_OK(c);
        if (M > 0) ACX_HIP(c, hipMemcpy(out_pos, d_pos, 4 * (size_t)M, hipMemcpyDeviceToHost));
        ACX_HIP(c, hipMemcpy(out_flag, d_flag, (size_t)n_rows, hipMemcpyDeviceToHost));
        return ACX_OK;
    });
}

int acx_topk_rows(acx_ctx *c, const float *scores, int64_t ld, int32_t n, int32_t n_rows, const int32_t *self, const int32_t *posn, int32_t k,
                  int32_t *out_idx, float *out_score)
{
    if (!c) return ACX_ERR_INVALID;
    int rc = rank_check_common(c, "topk_rows", scores, ld, n, n_rows, self, posn);
    if (rc != ACX_OK) return rc;
    if ((rc = rank_check_k(c, "topk_rows", k, n_rows, out_idx, out_score)) != ACX_OK) return rc;
    if (n_rows == 0) return ACX_OK;
    const int64_t fixed = 4 * (int64_t)n_rows + 4 * (int64_t)n;
    int32_t piece = 0;
    if ((rc = rank_piece_rows(c, "topk_rows", n, n_rows, 8 * (int64_t)k, fixed, &piece)) != ACX_OK) return rc;
    ACX_HIP(c, hipSetDevice(c->device));
    if ((rc = rank_lds_attr(c)) != ACX_OK) return rc;
    int P = 4;
    while (P < std::min<int>(k, n - 1)) P <<= 1;
    // self | posn | two result slots of `piece` rows (indices, scores)
    const size_t o_posn = 4 * (size_t)n_rows, o_res = o_posn + (posn ? 4 * (size_t)n : 0), slot_bytes = 8 * (size_t)k * piece,
                 total = o_res + 2 * slot_bytes;
    return with_device_block(c, "topk_rows", total, [&](char *d_tab) -> int {
        ACX_HIP(c, hipMemcpyAsync(d_tab, self, 4 * (size_t)n_rows, hipMemcpyHostToDevice, c->stream));
        if (posn) ACX_HIP(c, hipMemcpyAsync(d_tab + o_posn, posn, 4 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        const int32_t *d_self = reinterpret_cast<const int32_t *>(d_tab);
        const int32_t *d_posn = posn ? reinterpret_cast<const int32_t *>(d_tab + o_posn) : nullptr;
        const bool in_lds = n <= acx::RANK_ROW_LDS;
        const size_t lds = 12 * (size_t)P + acx::RANK_SELECT_LDS_FIXED + (in_lds ? 16 * (size_t)((n + 3) / 4) : 0);
        int p = 0;
        int rcp = rank_for_pieces(c, scores, ld, n, n_rows, piece, [&](const float *d_rows, int64_t ldd, int32_t r0, int32_t nr) -> int {
            // (the result slot alternates with the staging slot: its previous copy to the host was issued on the same stream)
            int32_t *d_idx = reinterpret_cast<int32_t *>(d_tab + o_res + (size_t)(p & 1) * slot_bytes);
            float *d_sc = reinterpret_cast<float *>(d_idx + (size_t)k * piece);
            ++p;
            {
                ProfScope ps(c, KS_TOPK, (int64_t)nr * n);
                ACX_LAUNCH_IN_LDS(topk_rows_kernel, in_lds, dim3((unsigned)nr), lds, d_rows, ldd, (int)n, d_self + r0, d_posn, (int)k, P, d_idx, d_sc);
            }
            ACX_HIP(c, hipMemcpyAsync(out_idx + (size_t)r0 * k, d_idx, 4 * (size_t)k * nr, hipMemcpyDeviceToHost, c->stream));
            ACX_HIP(c, hipMemcpyAsync(out_score + (size_t)r0 * k, d_sc, 4 * (size_t)k * nr, hipMemcpyDeviceToHost, c->stream));
            return ACX_OK;
        });
        if (rcp != ACX_OK) return rcp;
        ACX_LAUNCHES_OK(c);
        return ACX_OK;
    });
}

// Device state of one similarity-network-fusion run: P matrices (two generations), the kNN kernels,
// two N x N work buffers.
struct SnfRun {
    int m = 0, n = 0, K = 0;
    std::vector<DeviceBuffer<double>> cur, nxt, dV;
    std::vector<DeviceBuffer<int32_t>> dJ;
    DeviceBuffer<double> acc, ut, md;
};

static int snf_alloc(acx_ctx *c, SnfRun &R, int m, int n, int K)
{
    const size_t nn = (size_t)n * n;
    if (n > 65535) return fail(c, ACX_ERR_UNSUPPORTED, "snf_fuse: more than 65535 tracks are not supported on the device (one work-item per matrix cell)");
    const size_t need = ((size_t)2 * m + 2) * nn * sizeof(double) + (size_t)m * n * K * (sizeof(double) + sizeof(int32_t));
    if (need > (size_t)(0.8 * (double)c->total_mem)) return fail(c, ACX_ERR_NOMEM, "snf_fuse: matrices do not fit the device");
    R.m = m; R.n = n; R.K = K;
    R.cur.resize(m); R.nxt.resize(m); R.dV.resize(m); R.dJ.resize(m);
    ACX_HIP(c, R.acc.grow(nn));
    ACX_HIP(c, R.ut.grow(nn));
    ACX_HIP(c, R.md.grow((size_t)n));
    for (int i = 0; i < m; ++i) {
        ACX_HIP(c, R.cur[i].grow(nn));
        ACX_HIP(c, R.nxt[i].grow(nn));
        ACX_HIP(c, R.dV[i].grow((size_t)n * K));
        ACX_HIP(c, R.dJ[i].grow((size_t)n * K));
    }
    return ACX_OK;
}

// snf_ast_kernel<true> keeps one row of n doubles in LDS; beyond that the gathers go to global memory
static bool snf_row_fits_lds(int n) { return (size_t)n * sizeof(double) <= 160 * 1024 - 1024; }
static hipError_t snf_lds_optin(int n)
{
    return hipFuncSetAttribute(reinterpret_cast<const void *>(acx::snf_ast_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)((size_t)n * sizeof(double)));
}

// One update of the cross-diffusion:  acc = (sum of sp) * scale,  ut = acc S^T,  nxt = S ut (+ reg_diag on the diagonal),
// S = (dJ, dV).  The loop below and acx_snf_debug_update both launch it here, so that the tests see the product's launches.
static void snf_update(acx_ctx *c, const acx::SnfSrc &sp, double scale, double *acc, const int32_t *dJ, const double *dV, double *ut,
                       double *nxt, int n, int K, double reg_diag, bool ldsrow)
{
    const size_t nn = (size_t)n * n;
    hipLaunchKernelGGL(acx::snf_mean_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, c->stream, sp, scale, acc, (int64_t)nn);
    if (ldsrow)
        hipLaunchKernelGGL((acx::snf_ast_kernel<true>), dim3(n), dim3(256), (size_t)n * sizeof(double), c->stream, acc, dJ, dV, ut, n, K);
    else
        hipLaunchKernelGGL((acx::snf_ast_kernel<false>), dim3(n), dim3(256), 0, c->stream, acc, dJ, dV, ut, n, K);
    hipLaunchKernelGGL(acx::snf_sut_kernel, dim3(n), dim3(256), 0, c->stream, ut, dJ, dV, nxt, n, K, reg_diag);
}

// Where the stages of one matrix go on the host, as each kernel leaves them (any may be null): the product asks for W only
struct SnfTaps {
    double *S = nullptr, *md = nullptr, *W = nullptr;
    int32_t *J = nullptr;
    double *V = nullptr, *P = nullptr;
};

// One matrix of acx_snf_fuse_dists, from the host matrix `M` to P = row-normalised W in `cur` and the kNN kernel in (dJ, dV):
// getW (similarity_fusion.py:15-36: symmetrise, local scale from the K + 1 nearest, Gaussian kernel), getS (:124-144) as
// neighbour lists, getP (:101-122).  from_stage = 1 (tests): M is already the affinity matrix, getW is skipped.  `acc` is the
// staging buffer, `ut` holds S and then W.  The product entry point and acx_snf_debug_stages both launch the kernels here.
static hipError_t snf_prepare_dev(acx_ctx *c, double *acc, double *ut, double *md, int32_t *dJ, double *dV, double *cur, int n, int K,
                                  double mu, int from_stage, const SnfTaps &tap, bool lists = true);

static hipError_t snf_prepare(acx_ctx *c, const double *M, double *acc, double *ut, double *md, int32_t *dJ, double *dV, double *cur,
                              int n, int K, double mu, int from_stage, const SnfTaps &tap)
{
    const size_t nn = (size_t)n * n;
    hipError_t e = hipMemcpyAsync(from_stage == 0 ? acc : ut, M, nn * sizeof(double), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return e;
    return snf_prepare_dev(c, acc, ut, md, dJ, dV, cur, n, K, mu, from_stage, tap);
}

// The same behind the copy, for a matrix that is on the device already: in `acc` (from_stage = 0) or in `ut` (from_stage = 1).
// lists = false stops behind getW (the diagonal blocks of the cross-diffusion fusion, which take their lists from the whole W).
static hipError_t snf_prepare_dev(acx_ctx *c, double *acc, double *ut, double *md, int32_t *dJ, double *dV, double *cur, int n, int K,
                                  double mu, int from_stage, const SnfTaps &tap, bool lists)
{
    const size_t nn = (size_t)n * n;
    const dim3 tg((n + 31) / 32, (n + 31) / 32);
    const unsigned rows4 = (unsigned)((n + 3) / 4);
    hipError_t e = hipSuccess;
    if (from_stage == 0) {
        hipLaunchKernelGGL(acx::snf_sym_kernel, tg, dim3(256), 0, c->stream, acc, ut, n);
        if (tap.S) e = hipMemcpyAsync(tap.S, ut, nn * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        hipLaunchKernelGGL(acx::snf_localscale_kernel, dim3(rows4), dim3(256), 0, c->stream, ut, md, n, K);
        if (tap.md && e == hipSuccess) e = hipMemcpyAsync(tap.md, md, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        hipLaunchKernelGGL(acx::snf_affinity_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, c->stream, ut, md, n, mu);
    }
    if (tap.W && e == hipSuccess) e = hipMemcpyAsync(tap.W, ut, nn * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (lists) {
        hipLaunchKernelGGL(acx::snf_knn_kernel, dim3(rows4), dim3(256), 0, c->stream, ut, dJ, dV, n, K);
        hipLaunchKernelGGL(acx::snf_rownorm_kernel, dim3(n), dim3(256), 0, c->stream, ut, cur, n);
        if (tap.J && e == hipSuccess) e = hipMemcpyAsync(tap.J, dJ, (size_t)n * K * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
        if (tap.V && e == hipSuccess) e = hipMemcpyAsync(tap.V, dV, (size_t)n * K * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (tap.P && e == hipSuccess) e = hipMemcpyAsync(tap.P, cur, nn * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    }
    if (e == hipSuccess) e = hipGetLastError();
    return e;
}

// The cross-diffusion loop of doSimilarityFusionWs (similarity_fusion.py:146-186) on matrices that are
// already on the device: cur[i] = row-normalised W_i, (dJ[i], dV[i]) = its kNN kernel.  out = nullptr: the result stays in
// R.acc and the launches stay queued (the caller goes on with it on the device).
static int snf_loop(acx_ctx *c, SnfRun &R, int niters, double reg_diag, double *out)
{
    const int m = R.m, n = R.n, K = R.K;
    const size_t nn = (size_t)n * n;
    const bool ldsrow = snf_row_fits_lds(n);
    if (ldsrow) ACX_HIP(c, snf_lds_optin(n));
    for (int it = 0; it < niters; ++it) {
        // from the second sweep on the reference's two work lists alias: a matrix updated earlier in the
        // sweep is already seen by the later ones (similarity_fusion.py:179)
        std::vector<DeviceBuffer<double>> &src = it == 0 ? R.cur : R.nxt;
        for (int i = 0; i < m; ++i) {
            acx::SnfSrc sp;
            sp.count = 0;
            for (int k = 0; k < m; ++k)
                if (k != i) sp.p[sp.count++] = src[k];
            snf_update(c, sp, 1.0 / (double)(m - 1), R.acc, R.dJ[i], R.dV[i], R.ut, R.nxt[i], n, K, reg_diag, ldsrow);
        }
    }
    {
        acx::SnfSrc sp;
        sp.count = m;
        for (int k = 0; k < m; ++k) sp.p[k] = R.nxt[k];
        hipLaunchKernelGGL(acx::snf_mean_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, c->stream,
                           sp, 1.0 / (double)m, R.acc, (int64_t)nn);
    }
    ACX_HIP(c, hipGetLastError());
    if (!out) return ACX_OK;
    ACX_HIP(c, hipMemcpyAsync(out, R.acc, nn * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    ACX_HIP(c, hipStreamSynchronize(c->stream));
    return ACX_OK;
}

int acx_snf_fuse(acx_ctx *c, const double *const *Ws, const int32_t *const *Js, const double *const *Vs, int32_t m,
                 int32_t n, int32_t K, int32_t niters, double reg_diag, double *out)
{
    if (!c) return ACX_ERR_INVALID;
    if (!Ws || !Js || !Vs || !out || m < 2 || m > 8 || n < 1 || K < 1 || K > n || niters < 1)
        return fail(c, ACX_ERR_INVALID, "snf_fuse: bad argument (2 <= m <= 8, 1 <= K <= n, niters >= 1)");
    for (int i = 0; i < m; ++i)
        if (!Ws[i] || !Js[i] || !Vs[i]) return fail(c, ACX_ERR_INVALID, "snf_fuse: null matrix");
    for (int i = 0; i < m; ++i)
        for (int64_t e = 0; e < (int64_t)n * K; ++e)
            if (Js[i][e] < 0 || Js[i][e] >= n) return fail(c, ACX_ERR_INVALID, "snf_fuse: neighbour index out of range");
    ACX_HIP(c, hipSetDevice(c->device));
    SnfRun R;
    int rc = snf_alloc(c, R, m, n, K);
    if (rc != ACX_OK) return rc;
    const size_t nn = (size_t)n * n;
    hipError_t e = hipSuccess;
    for (int i = 0; i < m && e == hipSuccess; ++i) {
        e = hipMemcpyAsync(R.dV[i], Vs[i], (size_t)n * K * sizeof(double), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(R.dJ[i], Js[i], (size_t)n * K * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
        // P_i = row-normalised W_i (getP, similarity_fusion.py:101-122); `acc` is the staging buffer
        if (e == hipSuccess) e = hipMemcpyAsync(R.acc, Ws[i], nn * sizeof(double), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) hipLaunchKernelGGL(acx::snf_rownorm_kernel, dim3(n), dim3(256), 0, c->stream, R.acc, R.cur[i], n);
    }
    ACX_HIP(c, e);
    return snf_loop(c, R, niters, reg_diag, out);
}

int acx_snf_fuse_dists(acx_ctx *c, const double *const *Ds, int32_t m, int32_t n, int32_t K, int32_t niters, double reg_diag,
                       double mu, double *out, double *const *Ws_out)
{
    if (!c) return ACX_ERR_INVALID;
    if (!Ds || !out || m < 2 || m > 8 || n < 1 || K < 1 || K > n || niters < 1 || !(mu > 0.0))
        return fail(c, ACX_ERR_INVALID, "snf_fuse_dists: bad argument (2 <= m <= 8, 1 <= K <= n, niters >= 1, mu > 0)");
    if (K > 64) return fail(c, ACX_ERR_UNSUPPORTED, "snf_fuse_dists: more than 64 neighbours are not supported on the device");
    for (int i = 0; i < m; ++i)
        if (!Ds[i]) return fail(c, ACX_ERR_INVALID, "snf_fuse_dists: null matrix");
    ACX_HIP(c, hipSetDevice(c->device));
    SnfRun R;
    int rc = snf_alloc(c, R, m, n, K);
    if (rc != ACX_OK) return rc;
    hipError_t e = hipSuccess;
    for (int i = 0; i < m && e == hipSuccess; ++i) {
        SnfTaps tap;
        tap.W = Ws_out ? Ws_out[i] : nullptr;
        e = snf_prepare(c, Ds[i], R.acc, R.ut, R.md, R.dJ[i], R.dV[i], R.cur[i], n, K, mu, 0, tap);
    }
    ACX_HIP(c, e);
    return snf_loop(c, R, niters, reg_diag, out);
}

int acx_snf_debug_stages(acx_ctx *c, const double *M, int32_t n, int32_t K, double mu, int32_t from_stage, double *S, double *md,
                         double *W, int32_t *J, double *V, double *P)
{
    if (!c) return ACX_ERR_INVALID;
    if (!M || n < 1 || K < 1 || K > n || !(mu > 0.0) || from_stage < 0 || from_stage > 1)
        return fail(c, ACX_ERR_INVALID, "snf_debug_stages: bad argument (1 <= K <= n, mu > 0, from_stage 0 or 1)");
    if (K > 64) return fail(c, ACX_ERR_UNSUPPORTED, "snf_debug_stages: more than 64 neighbours are not supported on the device");
    ACX_HIP(c, hipSetDevice(c->device));
    SnfRun R;
    int rc = snf_alloc(c, R, 1, n, K);
    if (rc != ACX_OK) return rc;
    SnfTaps tap;
    if (from_stage == 0) { tap.S = S; tap.md = md; }
    tap.W = W; tap.J = J; tap.V = V; tap.P = P;
    // a slot of the lists that no lane writes shows as column -1 (and a NaN weight), not as whatever the block held before
    ACX_HIP(c, hipMemsetAsync(R.dJ[0], 0xff, (size_t)n * K * sizeof(int32_t), c->stream));
    ACX_HIP(c, hipMemsetAsync(R.dV[0], 0xff, (size_t)n * K * sizeof(double), c->stream));
    ACX_HIP(c, snf_prepare(c, M, R.acc, R.ut, R.md, R.dJ[0], R.dV[0], R.cur[0], n, K, mu, from_stage, tap));
    ACX_HIP(c, hipStreamSynchronize(c->stream));
    return ACX_OK;
}

int acx_snf_debug_update(acx_ctx *c, const double *const *srcs, int32_t m_src, int32_t n, int32_t K, double scale, const int32_t *J,
                         const double *V, double reg_diag, int32_t variant, const int32_t *rows, int32_t n_rows, double *acc_rows,
                         double *ut_rows, double *p_rows)
{
    if (!c) return ACX_ERR_INVALID;
    if (!srcs || !J || !V || m_src < 1 || m_src > 8 || n < 1 || K < 1 || K > n || variant < 0 || variant > 2 || n_rows < 0 ||
        (n_rows > 0 && !rows))
        return fail(c, ACX_ERR_INVALID, "snf_debug_update: bad argument (1 <= m_src <= 8, 1 <= K <= n, variant 0..2)");
    // (before anything of size n is read: the refusal needs no matrix)
    if (variant == 1 && !snf_row_fits_lds(n))
        return fail(c, ACX_ERR_UNSUPPORTED, "snf_debug_update: a row of n doubles does not fit the LDS");
    if (n > 65535) return fail(c, ACX_ERR_UNSUPPORTED, "snf_debug_update: more than 65535 tracks are not supported on the device");
    for (int k = 0; k < m_src; ++k)
        if (!srcs[k]) return fail(c, ACX_ERR_INVALID, "snf_debug_update: null matrix");
    for (int r = 0; r < n_rows; ++r)
        if (rows[r] < 0 || rows[r] >= n) return fail(c, ACX_ERR_INVALID, "snf_debug_update: row index out of range");
    for (int64_t e = 0; e < (int64_t)n * K; ++e)
        if (J[e] < 0 || J[e] >= n) return fail(c, ACX_ERR_INVALID, "snf_debug_update: neighbour index out of range");
    ACX_HIP(c, hipSetDevice(c->device));
    const size_t nn = (size_t)n * n;
    const size_t need = ((size_t)m_src + 3) * nn * sizeof(double) + (size_t)n * K * (sizeof(double) + sizeof(int32_t));
    if (need > (size_t)(0.8 * (double)c->total_mem)) return fail(c, ACX_ERR_NOMEM, "snf_debug_update: matrices do not fit the device");
    std::vector<DeviceBuffer<double>> src(m_src);
    DeviceBuffer<double> acc, ut, nxt, dV;
    DeviceBuffer<int32_t> dJ;
    ACX_HIP(c, acc.grow(nn));
    ACX_HIP(c, ut.grow(nn));
    ACX_HIP(c, nxt.grow(nn));
    ACX_HIP(c, dV.grow((size_t)n * K));
    ACX_HIP(c, dJ.grow((size_t)n * K));
    acx::SnfSrc sp;
    sp.count = m_src;
    for (int k = 0; k < m_src; ++k) {
        ACX_HIP(c, src[k].grow(nn));
        ACX_HIP(c, hipMemcpyAsync(src[k], srcs[k], nn * sizeof(double), hipMemcpyHostToDevice, c->stream));
        sp.p[k] = src[k];
    }
    ACX_HIP(c, hipMemcpyAsync(dV, V, (size_t)n * K * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ACX_HIP(c, hipMemcpyAsync(dJ, J, (size_t)n * K * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    const bool ldsrow = variant == 0 ? snf_row_fits_lds(n) : variant == 1;
    if (ldsrow) ACX_HIP(c, snf_lds_optin(n));
    snf_update(c, sp, scale, acc, dJ, dV, ut, nxt, n, K, reg_diag, ldsrow);
    ACX_HIP(c, hipGetLastError());
    for (int r = 0; r < n_rows; ++r) {
        const size_t at = (size_t)rows[r] * n, to = (size_t)r * n;
        if (acc_rows) ACX_HIP(c, hipMemcpyAsync(acc_rows + to, acc.get() + at, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (ut_rows) ACX_HIP(c, hipMemcpyAsync(ut_rows + to, ut.get() + at, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (p_rows) ACX_HIP(c, hipMemcpyAsync(p_rows + to, nxt.get() + at, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    ACX_HIP(c, hipStreamSynchronize(c->stream));
    return ACX_OK;
}

// ---------------------------------------------------------------------------------------
// EarlyFusion: the full cross-diffusion fusion for listed pairs (ef_crossfusion_kernels.hpp)
// ---------------------------------------------------------------------------------------
// Device state of a list: one SnfRun sized for the largest n of the list, the means of the three cross blocks, X.
struct XfRun {
    SnfRun R;
    DeviceBuffer<double> rc, X;          // [r x3 (M each)][c x3 (N each)];  X (M, N)
    acx::EfPair desc;                    // the plot's descriptor: the source of a queued copy, so it lives as long as the run
};

// the three triples of one pair on the device: f32, row pitches in floats
struct XfSrc {
    const float *SA[3], *SB[3], *C[3];
    int64_t ldA, ldB, ldC;
};

// where the intermediates of one pair go on the host (any may be null)
struct XfTaps {
    double *r = nullptr, *c = nullptr, *W = nullptr, *D = nullptr, *X = nullptr;
    uint32_t *bits = nullptr;
};

// k1 = int(K M / (M + N)), k2 = K - k1 (similarity_fusion.py:93-94); what np.partition refuses or divides by zero on is refused
static bool xf_split(int M, int N, int K, int &k1, int &k2)
{
    k1 = (int)((double)K * (double)M / (double)(M + N));
    k2 = K - k1;
    return k1 >= 1 && k2 >= 1 && k1 + 1 < M && k2 + 1 < N;
}

static std::string xf_split_text(int M, int N, int K)
{
    int k1, k2;
    (void)xf_split(M, N, K, k1, k2);
    return std::to_string(M) + " x " + std::to_string(N) + " blocks with K = " + std::to_string(K) + " give k1 = " + std::to_string(k1) + ", k2 = " +
           std::to_string(k2) + "; needed: 1 <= k1 < M - 1 and 1 <= k2 < N - 1";
}

static int xf_alloc(acx_ctx *c, XfRun &xr, int maxM, int maxN, int maxn, int K)
{
    int rc = snf_alloc(c, xr.R, 3, maxn, K);
    if (rc != ACX_OK) return rc;
    if ((rc = ensure(c, xr.rc, (size_t)3 * (maxM + maxN))) != ACX_OK) return rc;
    if ((rc = ensure(c, xr.X, (size_t)maxM * maxN)) != ACX_OK) return rc;
    if ((rc = ensure(c, c->d_efbits, (size_t)maxM * (round_up(maxN, 64) / 32))) != ACX_OK) return rc;
    if ((rc = ensure(c, c->d_efpd, (size_t)1)) != ACX_OK) return rc;
    return ensure(c, c->d_out, (size_t)4);
}

// Selection on X (xr.X, or the caller's matrix when the test entry put it there) and the Smith-Waterman on the bitmap: d_efbits
// holds the plot from word 0 on in the layout of a batch's plane, descriptor 0 of d_efpd says so; the score waits in d_out[0].
static int xf_select_sw(acx_ctx *c, XfRun &xr, int M, int N, int kbin, const XfTaps &tap)
{
    acx::EfPair &d = xr.desc;
    d = ef_one_pair(M, N, kbin);
    ACX_HIP(c, hipMemcpyAsync(c->d_efpd, &d, sizeof(d), hipMemcpyHostToDevice, c->stream));
    {
        ProfScope ps(c, KS_XFSELECT, (int64_t)M * N);
        hipLaunchKernelGGL(acx::xf_select_kernel, dim3((M + 3) / 4), dim3(256), 0, c->stream, xr.X, M, N, kbin, c->d_efbits);
    }
    if (tap.bits) ACX_HIP(c, hipMemcpyAsync(tap.bits, c->d_efbits, sizeof(uint32_t) * (size_t)M * (d.pitchC / 32), hipMemcpyDeviceToHost, c->stream));
    {
        ProfScope ps(c, KS_EFSW, (int64_t)M * N);
        if (N > 512) hipLaunchKernelGGL((acx::sw_bits_h16_kernel<16>), dim3(1, 1), dim3(64), 0, c->stream, c->d_efpd, c->d_efbits, c->d_out, 0);
        else hipLaunchKernelGGL((acx::sw_bits_h16_kernel<8>), dim3(1, 1), dim3(64), 0, c->stream, c->d_efpd, c->d_efbits, c->d_out, 0);
    }
    ACX_LAUNCHES_OK(c);
    return ACX_OK;
}

// One pair behind its GEMMs: W per feature (in R.nxt[f], which the loop only writes later), the lists and P of each, the loop,
// X, the bitmap and the score (queued; `score` is valid after the wait at the end).  The shape has passed xf_split.
static int xf_chain(acx_ctx *c, XfRun &xr, const XfSrc &s, int M, int N, int K, int kbin, int niters, double reg_diag,
                    const XfTaps &tap, float *score)
{
    SnfRun &R = xr.R;
    const int n = M + N;
    const double mu = 0.5;
    int k1, k2;
    (void)xf_split(M, N, K, k1, k2);
    R.n = n;
    const size_t nn = (size_t)n * n;
    double *r = xr.rc, *cm = xr.rc.get() + (size_t)3 * M;
    for (int f = 0; f < 3; ++f) {
        {
            ProfScope ps(c, KS_XFMEANS, (int64_t)M * N);
            hipLaunchKernelGGL(acx::xf_means_kernel, dim3((n + 3) / 4), dim3(256), 0, c->stream, s.C[f], M, N, s.ldC, k2, k1,
                               r + (size_t)f * M, cm + (size_t)f * N);
        }
        ProfScope ps(c, KS_XFAFFINITY, (int64_t)n * n);
        hipLaunchKernelGGL(acx::xf_cross_affinity_kernel, dim3((N + 31) / 32, (M + 31) / 32), dim3(256), 0, c->stream, s.C[f], M, N, s.ldC,
                           r + (size_t)f * M, cm + (size_t)f * N, mu, R.nxt[f].get());
        // the diagonal blocks: getW(S^A, k1) and getW(S^B, k2) on the three stage kernels of snf_prepare, then into place
        for (int side = 0; side < 2; ++side) {
            const int m = side ? N : M, kk = side ? k2 : k1;
            const unsigned g = (unsigned)(((size_t)m * m + 255) / 256);
            hipLaunchKernelGGL(acx::xf_widen_kernel, dim3(g), dim3(256), 0, c->stream, side ? s.SB[f] : s.SA[f], side ? s.ldB : s.ldA, m, R.acc.get());
            ACX_HIP(c, snf_prepare_dev(c, R.acc, R.ut, R.md, nullptr, nullptr, nullptr, m, kk, mu, 0, SnfTaps(), false));
            hipLaunchKernelGGL(acx::xf_place_kernel, dim3(g), dim3(256), 0, c->stream, R.ut.get(), m, R.nxt[f].get(), n, side ? M : 0);
        }
        if (tap.W) ACX_HIP(c, hipMemcpyAsync(tap.W + (size_t)f * nn, R.nxt[f], nn * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    {
        // doSimilarityFusionWs: getS and getP of every W (from_stage = 1 of snf_prepare, W where it is), then the loop
        ProfScope ps(c, KS_XFSNF, (int64_t)n * n);
        for (int f = 0; f < 3; ++f)
            ACX_HIP(c, snf_prepare_dev(c, nullptr, R.nxt[f], R.md, R.dJ[f], R.dV[f], R.cur[f], n, K, mu, 1, SnfTaps()));
        const int rc = snf_loop(c, R, niters, reg_diag, nullptr);
        if (rc != ACX_OK) return rc;
    }
    if (tap.D) ACX_HIP(c, hipMemcpyAsync(tap.D, R.acc, nn * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    {
        ProfScope ps(c, KS_XFX, (int64_t)M * N);
        hipLaunchKernelGGL(acx::xf_x_kernel, dim3((N + 31) / 32, (M + 31) / 32), dim3(256), 0, c->stream, R.acc.get(), M, N, xr.X.get());
    }
    if (tap.r) ACX_HIP(c, hipMemcpyAsync(tap.r, r, sizeof(double) * 3 * M, hipMemcpyDeviceToHost, c->stream));
    if (tap.c) ACX_HIP(c, hipMemcpyAsync(tap.c, cm, sizeof(double) * 3 * N, hipMemcpyDeviceToHost, c->stream));
    if (tap.X) ACX_HIP(c, hipMemcpyAsync(tap.X, xr.X, sizeof(double) * (size_t)M * N, hipMemcpyDeviceToHost, c->stream));
    const int rc = xf_select_sw(c, xr, M, N, kbin, tap);
    if (rc != ACX_OK) return rc;
    ACX_HIP(c, hipMemcpyAsync(score, c->d_out, sizeof(float), hipMemcpyDeviceToHost, c->stream));
    ACX_HIP(c, hipStreamSynchronize(c->stream));
    drain_profile(c);
    return ACX_OK;
}

static int xf_check_params(acx_ctx *c, const char *who, double kappa, int K, int niters)
{
    if (niters < 1) return fail(c, ACX_ERR_INVALID, std::string(who) + ": niters must be >= 1");
    if (K < 1) return fail(c, ACX_ERR_INVALID, std::string(who) + ": K must be >= 1");
    if (!(kappa >= 0.0)) return fail(c, ACX_ERR_INVALID, std::string(who) + ": kappa must be >= 0");
    if (K > 64) return fail(c, ACX_ERR_UNSUPPORTED, std::string(who) + ": more than 64 neighbours are not supported on the device");
    return ACX_OK;
}

// where the intermediates of the product path's one debug pair go (acx_ef_crossfusion_debug)
struct XfPairDebug {
    float *ssm_a, *ssm_b, *csm;
    XfTaps tap;
};

static int xf_pairs_impl(acx_ctx *c, const int32_t *pairs, int64_t Kp, const acx_ef_params *params, int32_t niters, double reg_diag,
                         float *out, const XfPairDebug *dbg)
{
    if (Kp < 0 || (Kp > 0 && (!pairs || !out)) || !params) return fail(c, ACX_ERR_INVALID, "ef_crossfusion: bad argument");
    int rc = xf_check_params(c, "ef_crossfusion", params->kappa, params->K, niters);
    if (rc != ACX_OK) return rc;
    if (Kp == 0) return ACX_OK;
    // the whole list before the first launch, on the caller's list
    int64_t good;                                // (this entry's own rules come before a later track without blocks)
    if ((rc = check_ef_pairs(c, pairs, Kp, &good)) != ACX_OK) return rc;
    const acx::EfLengths len{c->h_efoff.data(), c->ef_ntracks};
    int maxM = 0, maxN = 0, maxn = 0;
    for (int64_t k = 0; k < good; ++k) {
        const int64_t M = len.blocks(pairs[2 * k]), N = len.blocks(pairs[2 * k + 1]);
        if (M > acx::XF_MAXN || N > acx::XF_MAXN)
            return fail(c, ACX_ERR_UNSUPPORTED, "ef_crossfusion: the fusion needs the bit path: at most 1024 blocks (pair " + std::to_string(k) + ": " +
                                                    std::to_string(M) + " x " + std::to_string(N) + ")");
        int k1, k2;
        if (!xf_split((int)M, (int)N, params->K, k1, k2))
            return fail(c, ACX_ERR_UNSUPPORTED, "ef_crossfusion: pair " + std::to_string(k) + ": " + xf_split_text((int)M, (int)N, params->K));
        maxM = std::max(maxM, (int)M); maxN = std::max(maxN, (int)N); maxn = std::max(maxn, (int)(M + N));
    }
    if (good < Kp) return ef_short_pair(c, good);
    ACX_HIP(c, hipSetDevice(c->device));
    XfRun xr;
    if ((rc = xf_alloc(c, xr, maxM, maxN, maxn, params->K)) != ACX_OK) return rc;
    // the distances come from the product's own GEMM path: the pair and the two self pairs as one list of run_ef, whose
    // matrices stay in d_scratch (its statistics and scores are not used: K = 1 keeps them cheap, the GEMMs do not read K)
    const acx_ef_params gp{params->kappa, 1};
    std::vector<acx::EfPair> pd;
    for (int64_t k = 0; k < Kp; ++k) {
        const int32_t a = pairs[2 * k], b = pairs[2 * k + 1];
        const int32_t three[6] = {a, b, a, a, b, b};
        float sc[12];
        if ((rc = run_ef(c, three, 3, gp, sc, nullptr, nullptr, 0, 0, nullptr, nullptr, &pd)) != ACX_OK) return rc;
        if (pd.size() != 3) return fail(c, ACX_ERR_STATE, "ef_crossfusion: the GEMM batch returned " + std::to_string(pd.size()) + " descriptors");
        const int M = pd[0].M, N = pd[0].N;
        XfSrc s;
        s.ldC = pd[0].pitchC; s.ldA = pd[1].pitchC; s.ldB = pd[2].pitchC;
        for (int f = 0; f < 3; ++f) {
            s.C[f] = c->d_scratch + pd[0].offC + (int64_t)f * M * pd[0].pitchC;
            s.SA[f] = c->d_scratch + pd[1].offC + (int64_t)f * M * pd[1].pitchC;
            s.SB[f] = c->d_scratch + pd[2].offC + (int64_t)f * N * pd[2].pitchC;
        }
        if (dbg)
            for (int f = 0; f < 3; ++f) {
                if (dbg->csm) ACX_HIP(c, hipMemcpy2DAsync(dbg->csm + (size_t)f * M * N, sizeof(float) * N, s.C[f], sizeof(float) * s.ldC, sizeof(float) * N, M, hipMemcpyDeviceToHost, c->stream));
                if (dbg->ssm_a) ACX_HIP(c, hipMemcpy2DAsync(dbg->ssm_a + (size_t)f * M * M, sizeof(float) * M, s.SA[f], sizeof(float) * s.ldA, sizeof(float) * M, M, hipMemcpyDeviceToHost, c->stream));
                if (dbg->ssm_b) ACX_HIP(c, hipMemcpy2DAsync(dbg->ssm_b + (size_t)f * N * N, sizeof(float) * N, s.SB[f], sizeof(float) * s.ldB, sizeof(float) * N, N, hipMemcpyDeviceToHost, c->stream));
            }
        if ((rc = xf_chain(c, xr, s, M, N, params->K, acx::ef_kbin(params->kappa, N), niters, reg_diag, dbg ? dbg->tap : XfTaps(), out + k)) != ACX_OK) return rc;
    }
    return ACX_OK;
}

int acx_ef_crossfusion_pairs(acx_ctx *c, const int32_t *pairs, int64_t K_pairs, const acx_ef_params *params, int32_t niters,
                             double reg_diag, float *out)
{
    if (!c) return ACX_ERR_INVALID;
    return guarded(c, [&] { return xf_pairs_impl(c, pairs, K_pairs, params, niters, reg_diag, out, nullptr); });
}

int acx_ef_crossfusion_debug(acx_ctx *c, int32_t i, int32_t j, const acx_ef_params *params, int32_t niters, double reg_diag,
                             float *ssm_a, float *ssm_b, float *csm, double *W, double *D, double *X, uint32_t *bits, float *score)
{
    if (!c) return ACX_ERR_INVALID;
    const int32_t pr[2] = {i, j};
    float sc = 0.0f;
    XfPairDebug dbg{ssm_a, ssm_b, csm, XfTaps()};
    dbg.tap.W = W; dbg.tap.D = D; dbg.tap.X = X; dbg.tap.bits = bits;
    const int rc = guarded(c, [&] { return xf_pairs_impl(c, pr, 1, params, niters, reg_diag, &sc, &dbg); });
    if (rc == ACX_OK && score) *score = sc;
    return rc;
}

static int xf_matrices_impl(acx_ctx *c, const float *SA, const float *SB, const float *C, int32_t M, int32_t N, double kappa, int32_t K,
                            int32_t niters, double reg_diag, const XfTaps &tap, float *score)
{
    if (!SA || !SB || !C || M < 1 || N < 1) return fail(c, ACX_ERR_INVALID, "crossfusion_matrices: bad argument");
    int rc = xf_check_params(c, "crossfusion_matrices", kappa, K, niters);
    if (rc != ACX_OK) return rc;
    if (M > acx::XF_MAXN || N > acx::XF_MAXN)
        return fail(c, ACX_ERR_UNSUPPORTED, "crossfusion_matrices: more than 1024 rows or columns (the kernels hold a row in one wave)");
    int k1, k2;
    if (!xf_split(M, N, K, k1, k2)) return fail(c, ACX_ERR_UNSUPPORTED, "crossfusion_matrices: " + xf_split_text(M, N, K));
    ACX_HIP(c, hipSetDevice(c->device));
    XfRun xr;
    if ((rc = xf_alloc(c, xr, M, N, M + N, K)) != ACX_OK) return rc;
    const size_t na = (size_t)M * M, nb = (size_t)N * N, nc = (size_t)M * N;
    if ((rc = ensure(c, c->d_scratch, 3 * (na + nb + nc))) != ACX_OK) return rc;
    float *dA = c->d_scratch, *dB = dA + 3 * na, *dC = dB + 3 * nb;
    ACX_HIP(c, hipMemcpyAsync(dA, SA, sizeof(float) * 3 * na, hipMemcpyHostToDevice, c->stream));
    ACX_HIP(c, hipMemcpyAsync(dB, SB, sizeof(float) * 3 * nb, hipMemcpyHostToDevice, c->stream));
    ACX_HIP(c, hipMemcpyAsync(dC, C, sizeof(float) * 3 * nc, hipMemcpyHostToDevice, c->stream));
    XfSrc s;
    s.ldA = M; s.ldB = N; s.ldC = N;
    for (int f = 0; f < 3; ++f) { s.SA[f] = dA + f * na; s.SB[f] = dB + f * nb; s.C[f] = dC + f * nc; }
    float sc = 0.0f;
    if ((rc = xf_chain(c, xr, s, M, N, K, acx::ef_kbin(kappa, N), niters, reg_diag, tap, &sc)) != ACX_OK) return rc;
    if (score) *score = sc;
    return ACX_OK;
}

int acx_crossfusion_matrices(acx_ctx *c, const float *SA, const float *SB, const float *C, int32_t M, int32_t N, double kappa,
                             int32_t K, int32_t niters, double reg_diag, double *r, double *cm, double *W, double *D, double *X,
                             uint32_t *bits, float *score)
{
    if (!c) return ACX_ERR_INVALID;
    XfTaps tap;
    tap.r = r; tap.c = cm; tap.W = W; tap.D = D; tap.X = X; tap.bits = bits;
    return guarded(c, [&] { return xf_matrices_impl(c, SA, SB, C, M, N, kappa, K, niters, reg_diag, tap, score); });
}

static int xf_xsel_impl(acx_ctx *c, const double *X, int32_t M, int32_t N, double kappa, uint32_t *bits, float *score)
{
    if (!X || M < 1 || N < 1 || !(kappa >= 0.0)) return fail(c, ACX_ERR_INVALID, "xsel_binary_sw: bad argument");
    if (M > acx::XF_MAXN || N > acx::XF_MAXN)
        return fail(c, ACX_ERR_UNSUPPORTED, "xsel_binary_sw: more than 1024 rows or columns (the kernels hold a row in one wave)");
    ACX_HIP(c, hipSetDevice(c->device));
    XfRun xr;
    int rc;
    if ((rc = ensure(c, xr.X, (size_t)M * N)) != ACX_OK) return rc;
    if ((rc = ensure(c, c->d_efbits, (size_t)M * (round_up(N, 64) / 32))) != ACX_OK) return rc;
    if ((rc = ensure(c, c->d_efpd, (size_t)1)) != ACX_OK) return rc;
    if ((rc = ensure(c, c->d_out, (size_t)4)) != ACX_OK) return rc;
    ACX_HIP(c, hipMemcpyAsync(xr.X, X, sizeof(double) * (size_t)M * N, hipMemcpyHostToDevice, c->stream));
    XfTaps tap;
    tap.bits = bits;
    if ((rc = xf_select_sw(c, xr, M, N, acx::ef_kbin(kappa, N), tap)) != ACX_OK) return rc;
    float sc = 0.0f;
    ACX_HIP(c, hipMemcpyAsync(&sc, c->d_out, sizeof(float), hipMemcpyDeviceToHost, c->stream));
    ACX_HIP(c, hipStreamSynchronize(c->stream));
    drain_profile(c);
    if (score) *score = sc;
    return ACX_OK;
}

int acx_xsel_binary_sw(acx_ctx *c, const double *X, int32_t M, int32_t N, double kappa, uint32_t *bits, float *score)
{
    if (!c) return ACX_ERR_INVALID;
    return guarded(c, [&] { return xf_xsel_impl(c, X, M, N, kappa, bits, score); });
}

// ---------------------------------------------------------------------------------------
// appends and truncation: tracks behind an uploaded pool in O(new tracks) work
//
// An append (1) checks everything, (2) makes room in every block of the pool, derived ones included (grow_keep: the pool is
// the same pool afterwards), (3) writes the new tracks and their derived data BEHIND the pool's end, where nothing reads, and
// (4) moves the end: counts and host offsets.  A failure before (4) leaves the pool as it was: (2) carries the slack behind the
// end into every block it replaces, and after a failure inside (3), which writes over that slack, it is restored (*_seal), which
// is also all a truncate does besides moving the end back.
// ---------------------------------------------------------------------------------------

// Grow and keep: the block `b` gets room for `need` elements.  A block that is too small is replaced by one of max(need, 1.5 x capacity):
// allocated beside the old one, the first `keep` elements copied device to device on the library's stream, then the old one freed.
// `keep` counts whatever a reader may touch: the live elements and, where a block has slack behind its end, that slack.  A failure
// leaves the old block.
extern "C++" {
template <typename T>
static int grow_keep(acx_ctx *c, DeviceBuffer<T> &b, size_t keep, size_t need)
{
    if (need <= b.capacity()) return ACX_OK;
    const size_t ncap = std::max(need, b.capacity() + b.capacity() / 2);
    DeviceBuffer<T> fresh;
    const hipError_t e = fresh.grow(ncap);
    if (e != hipSuccess)
        return fail(c, ACX_ERR_NOMEM, "append: hipMalloc of " + std::to_string(ncap * sizeof(T)) + " bytes failed: " + hipGetErrorString(e));
    if (keep) ACX_HIP(c, hipMemcpyAsync(fresh.get(), b.get(), sizeof(T) * keep, hipMemcpyDeviceToDevice, c->stream));
    ACX_HIP(c, hipStreamSynchronize(c->stream));
    b = std::move(fresh);                                   // (frees the old block)
    return ACX_OK;
}
}  // extern "C++"

// What every append checks first: the arguments that all of them share, and the offsets of the new tracks (relative: offsets[0] == 0).
static int append_check(acx_ctx *c, const char *who, const void *data, const int64_t *offsets, int32_t n_new, int64_t n_old)
{
    if (!data) return fail(c, ACX_ERR_INVALID, std::string(who) + ": the feature pointer must not be NULL");
    if (n_new <= 0) return fail(c, ACX_ERR_INVALID, std::string(who) + ": n_new must be >= 1");
    if (n_old + n_new > 0x7fffffffLL) return fail(c, ACX_ERR_INVALID, std::string(who) + ": n_new takes the pool beyond 2^31 - 1 tracks");
    if (!offsets) return ACX_OK;                            // (one row per track)
    if (offsets[0] != 0) return fail(c, ACX_ERR_INVALID, std::string(who) + ": offsets[0] must be 0 (offsets are relative to the appended tracks)");
    for (int i = 0; i < n_new; ++i)
        if (offsets[i + 1] < offsets[i]) return fail(c, ACX_ERR_INVALID, std::string(who) + ": offsets must be non-decreasing");
    return ACX_OK;
}

// offsets [n0 + 1, n0 + n_new] of a device offset table from the new tracks' relative ones (entry n0 is the pool's end already)
static int append_offsets(acx_ctx *c, int64_t *d_off, int64_t n0, int64_t end0, const int64_t *rel, int32_t n_new, std::vector<int64_t> &abs)
{
    abs.resize((size_t)n_new + 1);
    for (int i = 0; i <= n_new; ++i) abs[i] = end0 + rel[i];
    ACX_HIP(c, hipMemcpyAsync(d_off + n0, abs.data(), sizeof(int64_t) * (n_new + 1), hipMemcpyHostToDevice, c->stream));
    ACX_HIP(c, hipStreamSynchronize(c->stream));           // (abs is pageable)
    return ACX_OK;
}

static void plan_forget(acx_ctx *c) { c->plan_len.clear(); c->plan_spec.algo = -1; }

// ---- f32 pool (Serra09 / ChenFusion) ----

// The slack behind the pool's end as an upload leaves it: POOL_SLACK zeroed frames behind the rotated and the f16 pool, +inf from the
// norm table's end up to `norm_hi` + POOL_SLACK (norm_hi: the farthest table end anything was written for).
static int s09_seal(acx_ctx *c, int64_t norm_hi)
{
    if (c->pool_tau < 1) return ACX_OK;
    const int64_t atotal = c->h_off[c->n_tracks];
    if (c->d_frot) ACX_HIP(c, hipMemsetAsync(c->d_frot + (POOL_SLACK + atotal) * acx::FROT, 0, sizeof(float) * POOL_SLACK * acx::FROT, c->stream));
    if (c->d_fh) ACX_HIP(c, hipMemsetAsync(c->d_fh + (POOL_SLACK + atotal) * acx::FH, 0, sizeof(_Float16) * POOL_SLACK * acx::FH, c->stream));
    if (c->d_normtab && c->normtab_m > 0) {
        const int64_t tot = c->h_noff[c->n_tracks];
        if (norm_hi >= tot)
            ACX_HIP(c, hipMemsetD32Async((hipDeviceptr_t)(c->d_normtab + POOL_SLACK + tot), 0x7f800000, (size_t)(norm_hi - tot + POOL_SLACK), c->stream));
    }
    ACX_HIP(c, hipStreamSynchronize(c->stream));
    return ACX_OK;
}

// What an append of `n_new` tracks adds to the f32 pool, worked out on the host before anything is touched.
struct S09Tail {
    int n0 = 0, n1 = 0;
    std::vector<int64_t> off0, aoff, noff;     // n_new + 1 absolute offsets each: uploaded pool, active pool, norm table
    int maxT = 1, maxM = 1;                    // longest new track of the active pool, in frames / embedded frames
    bool active = false, table = false;        // the pool has an active copy (dim 12) / a norm table to extend
};

// Steps (1) and (2) for the f32 pool: on return every block has room for the new tracks and d_toff0's tail is written.
static int s09_append_begin(acx_ctx *c, const char *who, const int64_t *rel, int32_t n_new, S09Tail &t)
{
    quiesce(c);                                 // qstream / qstream2 may still hold sweeps that read the blocks replaced below
    const int dim = c->dim, tau = c->pool_tau;
    t.n0 = c->n_tracks; t.n1 = t.n0 + n_new;
    ACX_HIP(c, c->d_planes.reset());            // (the planes' pitch is the pool's length: rebuilt by the next wide batch, ensure_planes)
    const int64_t total0 = c->h_off0[t.n0], total1 = total0 + rel[n_new];
    t.active = dim == acx::NBIN && tau >= 1 && c->d_frames0 && c->d_toff0;
    t.table = t.active && c->d_normtab && c->d_noff && c->normtab_m > 0;
    const int64_t atotal0 = t.active ? c->h_off[t.n0] : 0, tot0 = t.table ? c->h_noff[t.n0] : 0;
    t.off0.resize((size_t)n_new + 1); t.aoff.assign((size_t)n_new + 1, atotal0); t.noff.assign((size_t)n_new + 1, tot0);
    for (int i = 0; i <= n_new; ++i) t.off0[i] = total0 + rel[i];
    for (int i = 0; i < n_new && t.active; ++i) {
        const int64_t T = rel[i + 1] - rel[i], Ta = tau == 1 ? T : (T + tau - 1) / tau;
        if (Ta > 0x7fffffffLL) return fail(c, ACX_ERR_INVALID, std::string(who) + ": offsets: a track has more than 2^31 - 1 frames");
        t.aoff[i + 1] = t.aoff[i] + Ta;
        t.maxT = std::max<int>(t.maxT, (int)Ta);
        if (t.table) {
            const int Me = std::max<int>(0, (int)Ta - c->normtab_span);
            t.maxM = std::max(t.maxM, Me);
            t.noff[i + 1] = t.noff[i] + (int64_t)acx::NBIN * (Me + acx::NGUARD);
        }
    }
    const int64_t atotal1 = t.aoff[n_new], tot1 = t.noff[n_new];
    int rc;
    if ((rc = grow_keep(c, c->d_frames0, (size_t)total0 * dim, (size_t)std::max<int64_t>(1, total1) * dim)) != ACX_OK) return rc;
    if ((rc = grow_keep(c, c->d_toff0, (size_t)t.n0 + 1, (size_t)t.n1 + 1)) != ACX_OK) return rc;
    if (dim == acx::NBIN && c->d_gch && (rc = grow_keep(c, c->d_gch, (size_t)t.n0 * acx::NBIN, (size_t)t.n1 * acx::NBIN)) != ACX_OK) return rc;
    if (t.active && tau > 1) {                  // the decimated copy
        if ((rc = grow_keep(c, c->d_frames, (size_t)atotal0 * acx::NBIN, (size_t)std::max<int64_t>(1, atotal1) * acx::NBIN)) != ACX_OK) return rc;
        if ((rc = grow_keep(c, c->d_toff, (size_t)t.n0 + 1, (size_t)t.n1 + 1)) != ACX_OK) return rc;
    }
    // The rotated pool, the f16 pool and the norm table are kept WITH the slack behind their end (zeros / +inf, which the band
    // kernel's edge tiles of the last track read): a replaced block is then sealed as the old one was, and an append that fails
    // before it has written behind the end -- a non-finite value under REJECT, a later allocation -- needs no seal.
    if (t.active && c->d_frot &&
        (rc = grow_keep(c, c->d_frot, (size_t)(atotal0 + 2 * POOL_SLACK) * acx::FROT, (size_t)(std::max<int64_t>(1, atotal1) + 2 * POOL_SLACK) * acx::FROT)) != ACX_OK)
        return rc;
    if (t.active && c->d_fh &&
        (rc = grow_keep(c, c->d_fh, (size_t)(atotal0 + 2 * POOL_SLACK) * acx::FH, (size_t)(std::max<int64_t>(1, atotal1) + 2 * POOL_SLACK) * acx::FH)) != ACX_OK)
        return rc;
    if (t.table) {
        if ((rc = grow_keep(c, c->d_normtab, (size_t)(tot0 + 2 * POOL_SLACK), (size_t)(std::max<int64_t>(1, tot1) + 2 * POOL_SLACK))) != ACX_OK) return rc;
        if ((rc = grow_keep(c, c->d_noff, (size_t)t.n0 + 1, (size_t)t.n1 + 1)) != ACX_OK) return rc;
    }
    ACX_HIP(c, hipMemcpyAsync(c->d_toff0 + t.n0, t.off0.data(), sizeof(int64_t) * (n_new + 1), hipMemcpyHostToDevice, c->stream));
    ACX_HIP(c, hipStreamSynchronize(c->stream));
    return ACX_OK;
}

// Step (3) for the derived data -- the new frames are in d_frames0 behind the pool's end, scanned -- and step (4).
static int s09_append_derived(acx_ctx *c, const S09Tail &t)
{
    const int n_new = t.n1 - t.n0, tau = c->pool_tau;
    if (c->dim == acx::NBIN && c->d_gch) {
        hipLaunchKernelGGL(acx::chroma_profile_kernel, dim3((unsigned)((n_new + 15) / 16)), dim3(256), 0, c->stream,
                           c->d_frames0.get(), c->d_toff0 + t.n0, n_new, c->d_gch + (size_t)t.n0 * acx::NBIN);
        ACX_HIP(c, hipGetLastError());
    }
    if (!t.active) return ACX_OK;
    const int64_t a0 = t.aoff[0], a1 = t.aoff[n_new], nfr = a1 - a0;
    if (tau > 1) {
        ACX_HIP(c, hipMemcpyAsync(c->d_toff + t.n0, t.aoff.data(), sizeof(int64_t) * (n_new + 1), hipMemcpyHostToDevice, c->stream));
        if (nfr > 0) {
            hipLaunchKernelGGL(acx::decimate_kernel, dim3(n_new, (t.maxT * acx::NBIN + 255) / 256), dim3(256), 0, c->stream,
                               c->d_frames0.get(), c->d_toff0 + t.n0, c->d_toff + t.n0, c->d_frames.get(), tau);
            ACX_HIP(c, hipGetLastError());
        }
    }
    const float *tail = c->active_frames() + a0 * acx::NBIN;
    if (c->d_frot) {
        if (nfr > 0) {
            hipLaunchKernelGGL(acx::rotpool_kernel, dim3((unsigned)std::min<int64_t>((nfr * acx::FROT + 255) / 256, 1 << 22)), dim3(256), 0, c->stream,
                               tail, c->d_frot + (POOL_SLACK + a0) * acx::FROT, nfr);
            ACX_HIP(c, hipGetLastError());
        }
        ACX_HIP(c, hipMemsetAsync(c->d_frot + (POOL_SLACK + a1) * acx::FROT, 0, sizeof(float) * POOL_SLACK * acx::FROT, c->stream));
    }
    if (c->d_fh) {
        // ensure_f16pool's range check, on the new frames: they can only take the pool's largest magnitude UP, so the lower bound
        // holds as it did (fh_base_n) and the upper one is theirs to break.  Beyond the range the operand pool is dropped, so that
        // the next f16x2 call rebuilds it and refuses the pool in ensure_f16pool's own words.
        unsigned h_m = 0u;
        if (nfr > 0) {
            DeviceBuffer<unsigned> d_m;
            ACX_HIP(c, d_m.grow(1));
            ACX_HIP(c, hipMemsetAsync(d_m, 0, sizeof(unsigned), c->stream));
            hipLaunchKernelGGL(absmax_kernel, dim3((unsigned)std::min<int64_t>((nfr * acx::NBIN + 255) / 256, 4096)), dim3(256), 0, c->stream,
                               tail, nfr * acx::NBIN, d_m.get());
            ACX_HIP(c, hipMemcpyAsync(&h_m, d_m, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
            ACX_HIP(c, hipStreamSynchronize(c->stream));
        }
        float mx;
        memcpy(&mx, &h_m, sizeof(mx));
        if (c->fh_base_n < 0 || !(mx <= F16X2_MAX_MAX)) {
            ACX_HIP(c, c->d_fh.reset());
            c->fh_base_n = -1;
        } else {
            ACX_HIP(c, hipMemsetAsync(c->d_fh + (POOL_SLACK + a0) * acx::FH, 0, sizeof(_Float16) * (size_t)(nfr + POOL_SLACK) * acx::FH, c->stream));
            if (nfr > 0) {
                hipLaunchKernelGGL(acx::rotpool_f16_kernel, dim3((unsigned)std::min<int64_t>((nfr * 12 + 255) / 256, 1 << 22)), dim3(256), 0, c->stream,
                                   tail, c->d_fh + (POOL_SLACK + a0) * acx::FH, nfr);
                ACX_HIP(c, hipGetLastError());
            }
        }
    }
    if (t.table) {
        // +inf first: the new region with its guard entries, and the slack behind the new end
        const int64_t tot0 = t.noff[0], tot1 = t.noff[n_new];
        ACX_HIP(c, hipMemsetD32Async((hipDeviceptr_t)(c->d_normtab + POOL_SLACK + tot0), 0x7f800000, (size_t)(tot1 - tot0 + POOL_SLACK), c->stream));
        ACX_HIP(c, hipMemcpyAsync(c->d_noff + t.n0, t.noff.data(), sizeof(int64_t) * (n_new + 1), hipMemcpyHostToDevice, c->stream));
        bool handled = true;
        {
            ProfScope ps(c, KS_NORMS, 0);
#define ACX_CALL(M_) launch_normtab<M_>(c, t.maxM, c->normtab_span, t.n0, n_new)
            ACX_M_SWITCH(c->normtab_m, ACX_CALL)
#undef ACX_CALL
        }
        if (!handled) return fail(c, ACX_ERR_UNSUPPORTED, "serra09: this build of libacx has no band kernel for the norm table's m");
        ACX_HIP(c, hipGetLastError());
    }
    ACX_HIP(c, hipStreamSynchronize(c->stream));
    return ACX_OK;
}

static int s09_append_finish(acx_ctx *c, const S09Tail &t)
{
    const int n_new = t.n1 - t.n0;
    const int rc = s09_append_derived(c, t);
    if (rc != ACX_OK) {
        const std::string first = c->err;
        (void)s09_seal(c, t.noff[n_new]);
        c->err = first;
        return rc;
    }
    c->h_off0.insert(c->h_off0.end(), t.off0.begin() + 1, t.off0.end());
    if (t.active) c->h_off.insert(c->h_off.end(), t.aoff.begin() + 1, t.aoff.end());
    if (t.table) c->h_noff.insert(c->h_noff.end(), t.noff.begin() + 1, t.noff.end());
    c->n_tracks = t.n1;
    plan_forget(c);
    drain_profile(c);
    return ACX_OK;
}

int acx_pool_append(acx_ctx *c, const float *frames, const int64_t *offsets, int32_t n_new, int32_t dim)
{
    if (!c) return ACX_ERR_INVALID;
    if (!c->d_frames0) return fail(c, ACX_ERR_STATE, "pool_append: feature pool not uploaded (acx_upload_pool)");
    if (!offsets) return fail(c, ACX_ERR_INVALID, "pool_append: offsets must not be NULL");
    int rc;
    if ((rc = append_check(c, "pool_append", frames, offsets, n_new, c->n_tracks)) != ACX_OK) return rc;
    if (dim != c->dim) return fail(c, ACX_ERR_INVALID, "pool_append: dim is " + std::to_string(dim) + ", the pool's is " + std::to_string(c->dim));
    ACX_HIP(c, hipSetDevice(c->device));
    c->nf_zeroed = 0;
    S09Tail t;
    if ((rc = s09_append_begin(c, "pool_append", offsets, n_new, t)) != ACX_OK) return rc;
    const int64_t total0 = t.off0[0], nfr = offsets[n_new];
    if (nfr > 0) ACX_HIP(c, hipMemcpy(c->d_frames0 + total0 * dim, frames, sizeof(float) * nfr * dim, hipMemcpyHostToDevice));
    // (track_of over the tail of d_toff0: the track is named by its index in the pool after the append)
    if ((rc = scan_nonfinite(c, "pool_append", "frames", c->d_frames0 + total0 * dim, nfr * dim, dim, total0, c->d_toff0 + t.n0, n_new, false, t.n0)) != ACX_OK) return rc;
    return s09_append_finish(c, t);
}

int acx_pool_append_raw(acx_ctx *c, const float *raw, const int64_t *raw_offsets, int32_t n_new, int32_t dim, int32_t fac,
                        int64_t *pooled_offsets_out)
{
    if (!c) return ACX_ERR_INVALID;
    if (!c->d_frames0) return fail(c, ACX_ERR_STATE, "pool_append_raw: feature pool not uploaded (acx_upload_pool / acx_upload_raw_pool)");
    if (!raw_offsets) return fail(c, ACX_ERR_INVALID, "pool_append_raw: raw_offsets must not be NULL");
    int rc;
    if ((rc = append_check(c, "pool_append_raw", raw, raw_offsets, n_new, c->n_tracks)) != ACX_OK) return rc;
    if (dim != 12 || c->dim != 12) return fail(c, ACX_ERR_INVALID, "pool_append_raw: dim must be 12, and so must the pool's");
    if (fac < 1) return fail(c, ACX_ERR_INVALID, "pool_append_raw: fac (the downsample factor) must be >= 1");
    if (fac > acx::POOL_MAXFAC) return fail(c, ACX_ERR_UNSUPPORTED, "pool_append_raw: fac: downsample factors above 64 are not supported on the device");
    ACX_HIP(c, hipSetDevice(c->device));
    c->nf_zeroed = 0;
    std::vector<int64_t> poff((size_t)n_new + 1, 0);
    for (int i = 0; i < n_new; ++i) poff[i + 1] = poff[i] + (raw_offsets[i + 1] - raw_offsets[i] + fac - 1) / fac;
    S09Tail t;
    if ((rc = s09_append_begin(c, "pool_append_raw", poff.data(), n_new, t)) != ACX_OK) return rc;
    const int64_t total0 = t.off0[0];
    DeviceBuffer<int64_t> d_roff;
    DeviceBuffer<float> d_raw;                       // staging of one slice of raw chroma; the medians go straight behind the pool's end
    ACX_HIP(c, d_roff.grow((size_t)n_new + 1));
    ACX_HIP(c, hipMemcpy(d_roff, raw_offsets, sizeof(int64_t) * (n_new + 1), hipMemcpyHostToDevice));
    const int64_t budget = raw_slice_bytes(c);
    rc = for_track_slices(
        n_new, n_new, [&](int t0, int t1) { return (raw_offsets[t1] - raw_offsets[t0]) * 12 * (int64_t)sizeof(float) <= budget; },
        [&](int t0, int t1) -> int {
            const int64_t nraw = raw_offsets[t1] - raw_offsets[t0], npool = poff[t1] - poff[t0];
            if (npool <= 0) return ACX_OK;
            ACX_HIP(c, d_raw.grow((size_t)nraw * 12));
            ACX_HIP(c, hipMemcpyAsync(d_raw, raw + raw_offsets[t0] * 12, sizeof(float) * nraw * 12, hipMemcpyHostToDevice, c->stream));
            const int rcs = scan_nonfinite(c, "pool_append_raw", "raw chroma", d_raw.get(), nraw * 12, 12, raw_offsets[t0], d_roff.get(), n_new, false, t.n0);
            if (rcs != ACX_OK) return rcs;
            // pooled frames [p0, p1) of the pool after the append, found in the tail of d_toff0
            const int64_t p0 = total0 + poff[t0], p1 = total0 + poff[t1];
            hipLaunchKernelGGL(acx::pool_median_kernel, dim3((unsigned)((npool + acx::POOL_FPB - 1) / acx::POOL_FPB)), dim3(256), 0, c->stream,
                               d_raw.get(), raw_offsets[t0], d_roff.get(), c->d_toff0 + t.n0, n_new, p0, p1, fac, c->d_frames0 + p0 * 12);
            ACX_HIP(c, hipGetLastError());
            ACX_HIP(c, hipStreamSynchronize(c->stream));     // (the next slice reuses d_raw)
            return ACX_OK;
        });
    if (rc != ACX_OK) return rc;
    if ((rc = s09_append_finish(c, t)) != ACX_OK) return rc;
    if (pooled_offsets_out) memcpy(pooled_offsets_out, poff.data(), sizeof(int64_t) * (n_new + 1));
    return ACX_OK;
}

static int s09_truncate(acx_ctx *c, int32_t n)
{
    quiesce(c);
    const bool table = c->d_normtab && c->normtab_m > 0 && c->pool_tau >= 1;
    const int64_t norm_hi = table ? c->h_noff[c->n_tracks] : 0;
    c->n_tracks = n;
    c->h_off0.resize((size_t)n + 1);
    if (c->pool_tau >= 1) c->h_off.resize((size_t)n + 1);
    if (table) c->h_noff.resize((size_t)n + 1);
    ACX_HIP(c, c->d_planes.reset());            // (ensure_planes rebuilds them for the shorter pool)
    // the f16x2 range check must still hold for the tracks that stay: it does while they contain the ones it was made for
    if (c->d_fh && (c->fh_base_n < 0 || n < c->fh_base_n)) {
        ACX_HIP(c, c->d_fh.reset());
        c->fh_base_n = -1;
    }
    plan_forget(c);
    return s09_seal(c, norm_hi);
}

// ---- f64 pool (SiMPle) ----

int acx_pool_append_f64(acx_ctx *c, const double *frames, const int64_t *offsets, int32_t n_new, int32_t dim)
{
    if (!c) return ACX_ERR_INVALID;
    if (!c->d_frames64) return fail(c, ACX_ERR_STATE, "pool_append_f64: f64 feature pool not uploaded (acx_upload_pool_f64)");
    if (!offsets) return fail(c, ACX_ERR_INVALID, "pool_append_f64: offsets must not be NULL");
    int rc;
    if ((rc = append_check(c, "pool_append_f64", frames, offsets, n_new, c->n_tracks64)) != ACX_OK) return rc;
    if (dim != 12) return fail(c, ACX_ERR_INVALID, "pool_append_f64: dim must be 12");
    ACX_HIP(c, hipSetDevice(c->device));
    c->nf_zeroed = 0;
    quiesce(c);
    const int n0 = c->n_tracks64, n1 = n0 + n_new;
    const int64_t total0 = c->h_off64[n0], nfr = offsets[n_new], total1 = total0 + nfr;
    if ((rc = grow_keep(c, c->d_frames64, (size_t)total0 * 12, (size_t)std::max<int64_t>(1, total1) * 12)) != ACX_OK) return rc;
    if ((rc = grow_keep(c, c->d_toff64, (size_t)n0 + 1, (size_t)n1 + 1)) != ACX_OK) return rc;
    if ((rc = grow_keep(c, c->d_prof64, (size_t)n0 * 12, (size_t)n1 * 12)) != ACX_OK) return rc;
    if (c->d_wn64 && (rc = grow_keep(c, c->d_wn64, (size_t)total0, (size_t)std::max<int64_t>(1, total1))) != ACX_OK) return rc;
    std::vector<int64_t> abs;
    if ((rc = append_offsets(c, c->d_toff64, n0, total0, offsets, n_new, abs)) != ACX_OK) return rc;
    double *tail = c->d_frames64 + total0 * 12;
    if (nfr > 0) ACX_HIP(c, hipMemcpy(tail, frames, sizeof(double) * nfr * 12, hipMemcpyHostToDevice));
    if ((rc = scan_nonfinite(c, "pool_append_f64", "frames", tail, nfr * 12, 12, total0, c->d_toff64 + n0, n_new, false, n0)) != ACX_OK) return rc;
    std::vector<double> cleaned;
    if (c->nf_zeroed > 0) {                          // policy ZERO: the profile below sums what the device holds
        cleaned.resize((size_t)nfr * 12);
        ACX_HIP(c, hipMemcpy(cleaned.data(), tail, sizeof(double) * nfr * 12, hipMemcpyDeviceToHost));
        frames = cleaned.data();
    }
    // per-track chroma profile, as the upload sums it
    std::vector<double> prof((size_t)n_new * 12, 0.0);
    int maxn = 1;
    for (int t = 0; t < n_new; ++t) {
        maxn = std::max<int>(maxn, (int)std::min<int64_t>(offsets[t + 1] - offsets[t], 0x7fffffff));
        for (int64_t f = offsets[t]; f < offsets[t + 1]; ++f)
            for (int b = 0; b < 12; ++b) prof[(size_t)t * 12 + b] += frames[f * 12 + b];
    }
    ACX_HIP(c, hipMemcpy(c->d_prof64 + (size_t)n0 * 12, prof.data(), sizeof(double) * prof.size(), hipMemcpyHostToDevice));
    if (c->d_wn64 && c->wn64_L > 0) {
        if (nfr > 0) ACX_HIP(c, hipMemsetAsync(c->d_wn64 + total0, 0, sizeof(double) * nfr, c->stream));
        hipLaunchKernelGGL(acx::simple_winnorm_kernel, dim3(n_new, std::min(64, (maxn + 255) / 256)), dim3(256), 0, c->stream,
                           c->d_frames64, c->d_toff64 + n0, c->d_wn64, c->wn64_L);
        ACX_HIP(c, hipGetLastError());
        ACX_HIP(c, hipStreamSynchronize(c->stream));
    }
    c->h_off64.insert(c->h_off64.end(), abs.begin() + 1, abs.end());
    c->n_tracks64 = n1;
    plan_forget(c);
    return ACX_OK;
}

// ---- EarlyFusion block features ----

// The +32 rows of slack behind d_efn / d_efsc (a group of 16 is read at once), for a pool of nb rows
static int ef_seal(acx_ctx *c, int64_t nb)
{
    for (int k = 0; k < 2; ++k)
        if (c->d_efn[k]) ACX_HIP(c, hipMemsetAsync(c->d_efn[k] + nb, 0, sizeof(float) * 32, c->stream));
    for (int k = 0; k < 3; ++k)
        if (c->d_efsc[k]) ACX_HIP(c, hipMemsetAsync(c->d_efsc[k] + nb, 0, sizeof(float) * 32, c->stream));
    ACX_HIP(c, hipStreamSynchronize(c->stream));
    return ACX_OK;
}

int acx_ef_pool_append(acx_ctx *c, const float *mfccs, const float *ssms, const float *chromas, const double *chroma_med,
                       const int64_t *offsets, int32_t n_new)
{
    if (!c) return ACX_ERR_INVALID;
    if (c->ef_open) return fail(c, ACX_ERR_STATE, "ef_pool_append: a pool is still being filled (acx_ef_pool_end)");
    if (!c->d_ef[0] || c->ef_ntracks <= 0) return fail(c, ACX_ERR_STATE, "ef_pool_append: block-feature pool not uploaded (acx_ef_upload_pool)");
    if (!offsets) return fail(c, ACX_ERR_INVALID, "ef_pool_append: offsets must not be NULL");
    if (!mfccs || !ssms || !chromas) return fail(c, ACX_ERR_INVALID, "ef_pool_append: mfccs, ssms and chromas must not be NULL");
    int rc;
    if ((rc = append_check(c, "ef_pool_append", chroma_med, offsets, n_new, c->ef_ntracks)) != ACX_OK) return rc;
    ACX_HIP(c, hipSetDevice(c->device));
    c->nf_zeroed = 0;
    quiesce(c);
    const int n0 = c->ef_ntracks, n1 = n0 + n_new, fmt = c->ef_split_fmt, nt = fmt == 1 ? 2 : 3;
    const int64_t nb0 = c->h_efoff[n0], nbq = offsets[n_new], nb1 = nb0 + nbq;
    const int32_t *dims = c->ef_dims;
    for (int k = 0; k < 3; ++k) {
        if ((rc = grow_keep(c, c->d_ef[k], (size_t)nb0 * dims[k], (size_t)std::max<int64_t>(1, nb1) * dims[k])) != ACX_OK) return rc;
        if (c->d_efs[k] && (rc = grow_keep(c, c->d_efs[k], (size_t)nb0 * 3 * c->ef_kp[k], (size_t)std::max<int64_t>(1, nb1) * 3 * c->ef_kp[k])) != ACX_OK) return rc;
        // (kept with their 32 rows of slack: a failure before the row kernels below then leaves nothing to seal)
        if (c->d_efsc[k] && (rc = grow_keep(c, c->d_efsc[k], (size_t)nb0 + 32, (size_t)nb1 + 32)) != ACX_OK) return rc;
        if (k < 2 && (rc = grow_keep(c, c->d_efn[k], (size_t)nb0 + 32, (size_t)nb1 + 32)) != ACX_OK) return rc;
    }
    if ((rc = grow_keep(c, c->d_efmed, (size_t)12 * n0, (size_t)12 * n1)) != ACX_OK) return rc;
    if ((rc = grow_keep(c, c->d_efoff, (size_t)n0 + 1, (size_t)n1 + 1)) != ACX_OK) return rc;
    std::vector<int64_t> abs;
    if ((rc = append_offsets(c, c->d_efoff, n0, nb0, offsets, n_new, abs)) != ACX_OK) return rc;
    const float *src[3] = {mfccs, ssms, chromas};
    static const char *what[3] = {"mfcc blocks", "ssm blocks", "chroma blocks"};
    for (int k = 0; k < 3; ++k) {
        float *tail = c->d_ef[k] + nb0 * dims[k];
        if (nbq > 0) ACX_HIP(c, hipMemcpy(tail, src[k], sizeof(float) * nbq * dims[k], hipMemcpyDefault));
        if ((rc = scan_nonfinite(c, "ef_pool_append", what[k], tail, nbq * dims[k], dims[k], nb0, c->d_efoff + n0, n_new, false, n0)) != ACX_OK) return rc;
    }
    ACX_HIP(c, hipMemcpy(c->d_efmed + (size_t)12 * n0, chroma_med, sizeof(double) * 12 * n_new, hipMemcpyDefault));
    if ((rc = scan_nonfinite<double>(c, "ef_pool_append", "chroma median", c->d_efmed + (size_t)12 * n0, (int64_t)12 * n_new, 12, 0, nullptr, n_new, false, n0)) != ACX_OK) return rc;
    // norms, row scales and splits of rows [nb0, nb1): every one of these kernels works on a row by itself
    rc = [&]() -> int {
        if (nbq > 0) {
            const unsigned g = (unsigned)((nbq + 3) / 4);
            hipLaunchKernelGGL(acx::ef_rownorm_kernel, dim3(g), dim3(256), 0, c->stream, c->d_ef[2] + nb0 * dims[2], nbq, dims[2], 1, (float *)nullptr);
            for (int k = 0; k < 2; ++k)
                hipLaunchKernelGGL(acx::ef_rownorm_kernel, dim3(g), dim3(256), 0, c->stream, c->d_ef[k] + nb0 * dims[k], nbq, dims[k], 0, c->d_efn[k] + nb0);
            ACX_HIP(c, hipGetLastError());
            for (int k = 0; k < 3; ++k) {
                if (c->ef_kp[k] == 0 || !c->d_efs[k]) continue;
                if (fmt == 1)
                    hipLaunchKernelGGL(acx::ef_rowscale_kernel, dim3(g), dim3(256), 0, c->stream, c->d_ef[k] + nb0 * dims[k], c->d_efsc[k] + nb0, nbq, dims[k]);
                const int64_t nthr = nbq * c->ef_kp[k];
                hipLaunchKernelGGL(acx::ef_split_bf16_kernel, dim3((unsigned)std::min<int64_t>((nthr + 255) / 256, 1 << 22)), dim3(256), 0, c->stream,
                                   c->d_ef[k] + nb0 * dims[k], c->d_efs[k] + nb0 * nt * c->ef_kp[k], nbq, dims[k], c->ef_kp[k], k == 2 ? 1 : 0,
                                   fmt == 1 ? c->d_efsc[k] + nb0 : (const float *)nullptr);
                ACX_HIP(c, hipGetLastError());
            }
        }
        return ef_seal(c, nb1);
    }();
    if (rc != ACX_OK) {
        const std::string first = c->err;
        (void)ef_seal(c, nb0);
        c->err = first;
        return rc;
    }
    c->h_efoff.insert(c->h_efoff.end(), abs.begin() + 1, abs.end());
    c->ef_ntracks = n1;
    plan_forget(c);
    return ACX_OK;
}

// ---- FTM2D shingles ----

int acx_ftm2d_append_shingles(acx_ctx *c, const double *shingles, int32_t n_new, int32_t dim)
{
    if (!c) return ACX_ERR_INVALID;
    if (c->ftm_open) return fail(c, ACX_ERR_STATE, "ftm2d_append_shingles: a pool is still being filled (acx_ftm2d_pool_end)");
    if (!c->d_ftm || c->ftm_n <= 0) return fail(c, ACX_ERR_STATE, "ftm2d_append_shingles: no shingle pool (acx_ftm2d_pool_* or acx_ftm2d_upload_shingles)");
    int rc;
    if ((rc = append_check(c, "ftm2d_append_shingles", shingles, nullptr, n_new, c->ftm_n)) != ACX_OK) return rc;
    if (dim != c->ftm_dim) return fail(c, ACX_ERR_INVALID, "ftm2d_append_shingles: dim is " + std::to_string(dim) + ", the pool's is " + std::to_string(c->ftm_dim));
    ACX_HIP(c, hipSetDevice(c->device));
    quiesce(c);
    const size_t keep = (size_t)c->ftm_n * dim, add = (size_t)n_new * dim;
    if ((rc = grow_keep(c, c->d_ftm, keep, keep + add)) != ACX_OK) return rc;
    ACX_HIP(c, hipMemcpy(c->d_ftm + keep, shingles, sizeof(double) * add, hipMemcpyHostToDevice));
    c->ftm_n += n_new;
    plan_forget(c);
    return ACX_OK;
}

int acx_pool_truncate(acx_ctx *c, int32_t algo, int32_t n_tracks)
{
    if (!c) return ACX_ERR_INVALID;
    int n = 0;
    switch (algo) {
    case ACX_ALGO_SERRA09: case ACX_ALGO_CHENFUSION:
        if (!c->d_frames0) return fail(c, ACX_ERR_STATE, "pool_truncate: feature pool not uploaded (acx_upload_pool)");
        n = c->n_tracks; break;
    case ACX_ALGO_SIMPLE:
        if (!c->d_frames64) return fail(c, ACX_ERR_STATE, "pool_truncate: f64 feature pool not uploaded (acx_upload_pool_f64)");
        n = c->n_tracks64; break;
    case ACX_ALGO_EARLYFUSION:
        if (!c->d_ef[0] || c->ef_open || c->ef_ntracks <= 0) return fail(c, ACX_ERR_STATE, "pool_truncate: no finished block-feature pool (acx_ef_upload_pool / acx_ef_pool_end)");
        n = c->ef_ntracks; break;
    case ACX_ALGO_FTM2D:
        if (!c->d_ftm || c->ftm_open) return fail(c, ACX_ERR_STATE, "pool_truncate: no finished FTM2D shingle pool (acx_ftm2d_pool_end / acx_ftm2d_upload_shingles)");
        n = c->ftm_n; break;
    default: return fail(c, ACX_ERR_INVALID, "pool_truncate: algo: unknown algorithm");
    }
    if (n_tracks < 1 || n_tracks > n)
        return fail(c, ACX_ERR_INVALID, "pool_truncate: n_tracks must be in 1.." + std::to_string(n) + " (got " + std::to_string(n_tracks) + ")");
    if (n_tracks == n) return ACX_OK;
    ACX_HIP(c, hipSetDevice(c->device));
    switch (algo) {
    case ACX_ALGO_SERRA09: case ACX_ALGO_CHENFUSION: return s09_truncate(c, n_tracks);
    case ACX_ALGO_SIMPLE:
        quiesce(c);
        c->n_tracks64 = n_tracks;
        c->h_off64.resize((size_t)n_tracks + 1);
        break;
    case ACX_ALGO_EARLYFUSION:
        quiesce(c);
        c->ef_ntracks = n_tracks;
        c->h_efoff.resize((size_t)n_tracks + 1);
        plan_forget(c);
        return ef_seal(c, c->h_efoff.back());
    default:
        quiesce(c);
        c->ftm_n = n_tracks;
    }
    plan_forget(c);
    return ACX_OK;
}

// ---------------------------------------------------------------------------------------
// the N x N pair grid
// ---------------------------------------------------------------------------------------
static int pool_lengths(acx_ctx *c, int algo, std::vector<int64_t> &len)
{
    const std::vector<int64_t> *off = nullptr;
    int n = 0;
    switch (algo) {
    case ACX_ALGO_SERRA09: case ACX_ALGO_CHENFUSION:
        if (!c->d_frames0) return fail(c, ACX_ERR_STATE, "grid: feature pool not uploaded (acx_upload_pool)");
        off = &c->h_off0; n = c->n_tracks; break;
    case ACX_ALGO_SIMPLE:
        if (!c->d_frames64) return fail(c, ACX_ERR_STATE, "grid: f64 feature pool not uploaded (acx_upload_pool_f64)");
        off = &c->h_off64; n = c->n_tracks64; break;
    case ACX_ALGO_EARLYFUSION:
        if (!c->d_ef[0] || c->ef_open) return fail(c, ACX_ERR_STATE, "grid: block-feature pool not uploaded (acx_ef_upload_pool)");
        off = &c->h_efoff; n = c->ef_ntracks; break;
    case ACX_ALGO_FTM2D:       // one shingle per track: every pair costs the same
        if (!c->d_ftm || c->ftm_open) return fail(c, ACX_ERR_STATE, "grid: FTM2D shingle pool not uploaded (acx_ftm2d_pool_* / acx_ftm2d_upload_shingles)");
        len.assign((size_t)c->ftm_n, 1);
        return ACX_OK;
    default: return fail(c, ACX_ERR_INVALID, "grid: unknown algorithm");
    }
    len.resize(n);
    for (int i = 0; i < n; ++i) len[i] = (*off)[i + 1] - (*off)[i];
    return ACX_OK;
}

int acx_grid_plan(const int64_t *lengths, int32_t n_tracks, const acx_grid_spec *spec, acx_grid_tile *tiles,
                  int64_t capacity, int64_t *n_tiles, int64_t *floats_per_rank, double *cost_per_rank)
{
    if (!lengths || n_tracks < 1 || !acx::grid_spec_ok(spec)) return ACX_ERR_INVALID;
    std::vector<acx_grid_tile> t;
    std::vector<int64_t> fl;
    std::vector<double> co;
    acx::grid_plan(lengths, n_tracks, *spec, t, fl, co);
    if (n_tiles) *n_tiles = (int64_t)t.size();
    if (tiles) {
        if (capacity < (int64_t)t.size()) return ACX_ERR_INVALID;
        std::copy(t.begin(), t.end(), tiles);
    }
    for (int r = 0; r < spec->world; ++r) {
        if (floats_per_rank) floats_per_rank[r] = fl[r];
        if (cost_per_rank) cost_per_rank[r] = co[r];
    }
    return ACX_OK;
}

// The Serra09 batch plan of a pair list without a device: run_serra09_impl's own checks, packing, sort and kernel choice
// (serra09_plan.hpp), one record per pair.  Messages of a refused list: acx_last_error(NULL).
int acx_serra09_plan(const int64_t *lengths, int32_t n_tracks, const int32_t *pairs, int64_t K, const acx_serra09_params *params,
                     int64_t scratch_limit, acx_serra09_plan_rec *out)
{
    if (!lengths || n_tracks < 1 || K < 0 || (K > 0 && (!pairs || !out)) || !params) return ACX_ERR_INVALID;
    int rc = check_params(nullptr, *params);
    if (rc != ACX_OK) return rc;
    std::vector<int64_t> off((size_t)n_tracks + 1, 0);
    for (int t = 0; t < n_tracks; ++t) off[t + 1] = off[t] + std::max<int64_t>(lengths[t], 0);
    const acx::Serra09Lengths len{off.data(), n_tracks, params->tau};
    const char *env = getenv("ACX_SCRATCH_GB");
    const int64_t limit_floats = scratch_limit > 0 ? scratch_limit / 4
                                 : (env && atof(env) > 0 ? (int64_t)(atof(env) * (double)(1ull << 30)) / 4 : INT64_MAX / 4);
    if ((rc = validate_serra09_pairs(nullptr, len, pairs, K, *params, false, limit_floats)) != ACX_OK) return rc;
    std::vector<PairDesc> pd, tmp;
    std::vector<int> perm;
    int64_t k0 = 0;
    for (int batch = 0; k0 < K; ++batch) {
        acx::Serra09Arena used;
        const int64_t k = acx::serra09_pack_batch(len, pairs, k0, K, *params, false, limit_floats, pd, used);
        if (k == k0) return ACX_ERR_STATE;
        const acx::Serra09Sort srt = acx::serra09_sort_batch(pd, tmp, perm, params->m);
        for (int cl = 0; cl <= acx::SERRA09_NC; ++cl) {
            const acx::Serra09Sweep sw = acx::serra09_sweep(cl);
            for (int k2 = srt.cls_begin[cl]; k2 < srt.cls_begin[cl + 1]; ++k2) {
                acx_serra09_plan_rec &r = out[k0 + perm[k2]];
                const bool band = cl < acx::SERRA09_NC;
                r.Mq = pd[k2].Mq; r.Mr = pd[k2].Mr;
                r.batch = batch;
                r.cr = cl; r.cq = band ? acx::serra09_row_class(pd[k2].Mq) : acx::SERRA09_NC;
                r.row_family = band ? acx::serra09_band_family(r.cr, params->m, params->arith) : ACX_SERRA09_FAMILY_STREAMING;
                r.col_family = band ? acx::serra09_band_family(r.cq, params->m, params->arith) : ACX_SERRA09_FAMILY_STREAMING;
                r.sweep_cols = sw.cols; r.sweep_pack = sw.pack;
            }
        }
        k0 = k;
    }
    return ACX_OK;
}

const char *acx_serra09_family_name(int32_t family, int32_t m) { return acx::serra09_family_name(family, m); }

// The EarlyFusion batch plan of a pair list without a device: acx_earlyfusion_pairs' run order and run_ef_impl's own checks, sizes,
// packing and kernel choice (ef_plan.hpp), one record per pair.  Messages of a refused list: acx_last_error(NULL).
int acx_ef_plan(const int64_t *blocks, int32_t n_tracks, const int32_t *pairs, int64_t K, const acx_ef_params *params, int64_t scratch_limit,
                int32_t keep_fused, acx_ef_plan_rec *out)
{
    if (!blocks || n_tracks < 1 || K < 0 || (K > 0 && (!pairs || !out)) || !params) return ACX_ERR_INVALID;
    if (!(params->kappa >= 0.0)) return fail(nullptr, ACX_ERR_INVALID, "earlyfusion: kappa must be >= 0");
    if (params->K < 1) return fail(nullptr, ACX_ERR_INVALID, "earlyfusion: K must be >= 1");
    std::vector<int64_t> off((size_t)n_tracks + 1, 0);
    for (int t = 0; t < n_tracks; ++t) off[t + 1] = off[t] + std::max<int64_t>(blocks[t], 0);
    const acx::EfLengths len{off.data(), n_tracks};
    int rc = ef_check_text(nullptr, acx::ef_check_pairs(len, pairs, K));
    if (rc != ACX_OK) return rc;
    std::vector<int64_t> order;
    std::vector<int32_t> sp;
    const bool sorted = acx::ef_run_order(pairs, K, order, sp);
    const int32_t *run = sorted ? pairs : sp.data();
    const char *env = getenv("ACX_SCRATCH_GB");
    const int64_t limit_floats = scratch_limit > 0 ? scratch_limit / 4
                                 : (env && atof(env) > 0 ? (int64_t)(atof(env) * (double)(1ull << 30)) / 4 : INT64_MAX / 4);
    const acx::EfMode mode = acx::ef_mode(len, run, K, params->K, keep_fused != 0);
    const acx::EfSizes sz = acx::ef_batch_floats(len, run, K, params->kappa, mode, limit_floats);
    if (sz.too_big >= 0) return fail(nullptr, ACX_ERR_NOMEM, "earlyfusion: pair " + std::to_string(sz.too_big) + " does not fit the scratch limit");
    std::vector<acx::EfPair> pd;
    int64_t k0 = 0;
    for (int batch = 0; k0 < K; ++batch) {
        acx::EfArena used;
        const int64_t k1 = acx::ef_pack_batch(len, run, k0, K, *params, mode, sz.batch_floats, pd, used);
        if (k1 == k0) return ACX_ERR_STATE;
        const acx::EfBatchKernels kn = acx::ef_batch_kernels(used.maxM, used.maxN, params->K, mode, false);
        for (int64_t k = k0; k < k1; ++k) {
            const acx::EfPair &d = pd[(size_t)(k - k0)];
            acx_ef_plan_rec &r = out[sorted ? k : order[(size_t)k]];
            r.M = d.M; r.N = d.N; r.kbin = d.kbin;
            r.batch = batch;
            r.path = mode.bits_path ? 0 : 1;
            r.row_kernel = kn.row; r.col_kernel = kn.col; r.fuse_kernel = kn.fuse; r.sw_kernel = kn.sw;
            r.reserved = 0;
            r.run_pos = k;
            r.need = acx::ef_pair_floats(d, mode.keep_f);
        }
        k0 = k1;
    }
    return ACX_OK;
}

const char *acx_ef_kernel_name(int32_t stage, int32_t kernel) { return acx::ef_kernel_name(stage, kernel); }

int64_t acx_serra09_fast_tail_launches(void) { return (int64_t)acx::fast_tail_launches(); }
int64_t acx_serra09_plane_launches(void) { return (int64_t)acx::plane_launches(); }

int acx_serra09_fast_tail(const acx_serra09_params *params, int32_t n_cells, int32_t role, int32_t debug)
{
    if (!params || n_cells < 1 || check_params(nullptr, *params) != ACX_OK) return ACX_ERR_INVALID;
    const int cl = acx::serra09_row_class(n_cells);
    if (cl >= acx::SERRA09_NC || params->m > acx::MAX_M) return 0;      // the streaming kernels
    const bool dbg = debug != 0;
    return acx::serra09_fast_tail_params(*params, acx::serra09_band_family(cl, params->m, params->arith), role, dbg && role == 0, dbg, true) &&
           acx::serra09_fast_tail_row(acx::pct_position(n_cells, params->kappa, params->pct_mode), n_cells) ? 1 : 0;
}

int acx_pool_lengths(acx_ctx *c, int32_t algo, int64_t *lengths, int32_t capacity, int32_t *n_tracks)
{
    if (!c) return ACX_ERR_INVALID;
    std::vector<int64_t> len;
    const int rc = pool_lengths(c, algo, len);
    if (rc != ACX_OK) return rc;
    if (n_tracks) *n_tracks = (int32_t)len.size();
    if (lengths) {
        if (capacity < (int32_t)len.size()) return fail(c, ACX_ERR_INVALID, "pool_lengths: buffer too small");
        std::copy(len.begin(), len.end(), lengths);
    }
    return ACX_OK;
}

// The plan of (pool lengths, spec), cached in the context: acx_grid_run is called once per slice of tiles
// (bench.py: once per step) and the plan is the same every time.
static const std::vector<acx_grid_tile> &cached_plan(acx_ctx *c, const std::vector<int64_t> &len, const acx_grid_spec &spec)
{
    const acx_grid_spec &q = c->plan_spec;
    if (q.algo != spec.algo || q.symmetric != spec.symmetric || q.tile != spec.tile || q.world != spec.world || c->plan_len != len) {
        std::vector<int64_t> fl;
        std::vector<double> co;
        acx::grid_plan(len.data(), (int)len.size(), spec, c->plan_tiles, fl, co);
        c->plan_len = len;
        c->plan_spec = spec;
    }
    return c->plan_tiles;
}

// SiMPle over a slice of tiles, everything on the device: pairs enumerated by grid_pairs_kernel (column-major
// inside a tile = sorted by the second track), simple_kernel, then the f64 -> f32 scatter into the score buffer.
// Nothing comes back to the host and the host waits for nothing between chunks.
static int run_simple_tiles(acx_ctx *c, const std::vector<acx_grid_tile> &mine, int symmetric, const acx_simple_params &sp, float *d_scores)
{
    size_t smem = 0;
    int rc = simple_front(c, sp.sslen, [&](auto visit) {
        for (const acx_grid_tile &t : mine) {
            for (int tr = t.row0; tr < t.row0 + t.rows; ++tr) visit(tr);
            for (int tr = t.col0; tr < t.col0 + t.cols; ++tr) visit(tr);
        }
    }, &smem);
    if (rc != ACX_OK) return rc;
    const int64_t CHUNK = (int64_t)1 << 22;
    std::vector<TileDev> td;
    size_t t0 = 0;
    while (t0 < mine.size()) {
        td.clear();
        int64_t n = 0, maxP = 0;
        size_t t1 = t0;
        while (t1 < mine.size()) {
            const acx_grid_tile &t = mine[t1];
            const int64_t P = tile_pair_count(t.rows, t.cols, t.diagonal, symmetric);
            if (t1 > t0 && n + P > CHUNK) break;
            if (P > 0) { td.push_back(TileDev{t.row0, t.col0, t.rows, t.cols, t.diagonal, 0, t.offset, n}); maxP = std::max(maxP, P); }
            n += P;
            ++t1;
        }
        if (n > 0) {
            if (n > 0x7fffffff) return fail(c, ACX_ERR_UNSUPPORTED, "simple: a single tile holds more than 2^31 pairs");
            if ((rc = ensure(c, c->d_pairs, (size_t)2 * n)) != ACX_OK) return rc;
            if ((rc = ensure(c, c->d_out64, (size_t)n)) != ACX_OK) return rc;
            if ((rc = ensure(c, c->d_idx, (size_t)n)) != ACX_OK) return rc;
            if ((rc = upload_tiles(c, td.data(), sizeof(TileDev) * td.size())) != ACX_OK) return rc;
            hipLaunchKernelGGL(grid_pairs_kernel, dim3((unsigned)std::min<int64_t>((maxP + 255) / 256, 256), (unsigned)td.size()), dim3(256), 0,
                               c->stream, reinterpret_cast<const TileDev *>(c->d_tiles.get()), symmetric, 1, c->d_pairs, c->d_idx);
            {
                ProfScope ps(c, KS_SIMPLE, n);
                if ((rc = launch_simple_sslen(c, sp.sslen, (int)n, smem, sp.oti)) != ACX_OK) return rc;
            }
            hipLaunchKernelGGL(scatter_f64_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->d_out64, c->d_idx, d_scores, (int)n);
            ACX_HIP(c, hipGetLastError());
        }
        t0 = t1;
    }
    return ACX_OK;
}

// FTM2D over a slice of tiles: every tile cut into 64 x 64 blocks of pairs (the lower blocks of a symmetric diagonal tile
// hold no pair and are left out), one workgroup per block, scores straight into d_scores.  No pair list anywhere.
static int run_ftm2d_tiles(acx_ctx *c, const std::vector<acx_grid_tile> &mine, int symmetric, float *d_scores)
{
    std::vector<acx::FtmTileItem> items;
    for (const acx_grid_tile &t : mine)
        for (int r0 = 0; r0 < t.rows; r0 += acx::FTM_TM)
            for (int c0 = 0; c0 < t.cols; c0 += acx::FTM_TM) {
                if (t.diagonal && symmetric && r0 > c0) continue;
                items.push_back(acx::FtmTileItem{t.row0, t.col0, t.rows, t.cols, r0, c0, t.diagonal, 0, t.offset});
            }
    if (items.empty()) return ACX_OK;
    const int rc = upload_tiles(c, items.data(), sizeof(acx::FtmTileItem) * items.size());
    if (rc != ACX_OK) return rc;
    hipLaunchKernelGGL(acx::ftm2d_tile_kernel, dim3((unsigned)items.size()), dim3(256), 0, c->stream, c->d_ftm, c->ftm_dim,
                       reinterpret_cast<const acx::FtmTileItem *>(c->d_tiles.get()), symmetric, d_scores);
    ACX_HIP(c, hipGetLastError());
    return ACX_OK;
}

// A pair list whose scores stay on the device, a chunk at a time: the chunk's pairs to c->d_pairs, its destinations to
// c->d_idx, then score(n) -- the pair kernel into d_out (room for a chunk) and the scatter from there to the destinations.
extern "C++" {
template <typename T, typename S>
static int run_list_chunks(acx_ctx *c, const int32_t *pairs, const int64_t *idx, int64_t K, DeviceBuffer<T> &d_out, S score)
{
    const int64_t CHUNK = (int64_t)1 << 22;
    int rc;
    if ((rc = ensure(c, c->d_pairs, (size_t)2 * std::min(K, CHUNK))) != ACX_OK) return rc;
    if ((rc = ensure(c, d_out, (size_t)std::min(K, CHUNK))) != ACX_OK) return rc;
    for (int64_t k0 = 0; k0 < K; k0 += CHUNK) {
        const int n = (int)std::min(CHUNK, K - k0);
        ACX_HIP(c, hipMemcpyAsync(c->d_pairs, pairs + 2 * k0, sizeof(int32_t) * 2 * n, hipMemcpyHostToDevice, c->stream));
        if ((rc = stage_idx(c, idx + k0, n)) != ACX_OK) return rc;
        if ((rc = score(n)) != ACX_OK) return rc;
        ACX_LAUNCHES_OK(c);
        ACX_HIP(c, hipStreamSynchronize(c->stream));      // (the pinned staging of the destinations is reused by the next chunk)
    }
    return ACX_OK;
}
}  // extern "C++"

// SiMPle: simple_kernel as acx_simple_pairs launches it, then the f64 -> f32 scatter of the grid path.
static int run_simple_list(acx_ctx *c, const int32_t *pairs, const int64_t *idx, int64_t K, const acx_simple_params &sp, float *d_scores)
{
    size_t smem = 0;
    const int rc = simple_front(c, sp.sslen, [&](auto visit) { for (int64_t k = 0; k < 2 * K; ++k) visit(pairs[k]); }, &smem);
    if (rc != ACX_OK) return rc;
    return run_list_chunks(c, pairs, idx, K, c->d_out64, [&](int n) -> int {
        {
            ProfScope ps(c, KS_SIMPLE, n);
            const int rc2 = launch_simple_sslen(c, sp.sslen, n, smem, sp.oti);
            if (rc2 != ACX_OK) return rc2;
        }
        hipLaunchKernelGGL(scatter_f64_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->d_out64, c->d_idx, d_scores, n);
        return ACX_OK;
    });
}

// FTM2D: ftm2d_pairs_kernel as acx_ftm2d_pairs launches it (the same accumulation, the same bits), then the scatter
// of the grid path.
static int run_ftm2d_list(acx_ctx *c, const int32_t *pairs, const int64_t *idx, int64_t K, float *d_scores)
{
    return run_list_chunks(c, pairs, idx, K, c->d_out, [&](int n) -> int {
        {
            ProfScope ps(c, KS_FTMPAIRS, n);
            hipLaunchKernelGGL(acx::ftm2d_pairs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->d_ftm, c->ftm_dim,
                               c->d_pairs, (int64_t)n, c->d_out);
        }
        hipLaunchKernelGGL(scatter_scores_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->d_out, c->d_idx, d_scores, n, 1);
        return ACX_OK;
    });
}

// Lowers the scratch limit a caller set by `bytes` (device memory the call holds beside the pair kernels' arenas) for
// the length of a scope.
struct ScratchReserve {
    acx_ctx *c; int64_t saved;
    ScratchReserve(acx_ctx *c_, int64_t bytes) : c(c_), saved(c_->scratch_limit) { if (saved > 0) c->scratch_limit = std::max<int64_t>(1, saved - bytes); }
    ~ScratchReserve() { c->scratch_limit = saved; }
};

// The one place where an ACX_ALGO_* value and its params become a runner that leaves the scores of a pair list on the
// device: pair k's planes at d_dst[idx[k] ...].  The Serra09 / ChenFusion / EarlyFusion kernels batch within the scratch
// limit less reserve_bytes.  Nothing here waits for the stream beyond what the runners do themselves.
static int run_pair_list(acx_ctx *c, int algo, const void *params, const int32_t *pairs, const int64_t *idx, int64_t K, float *d_dst,
                         int64_t reserve_bytes)
{
    if (algo == ACX_ALGO_FTM2D) return run_ftm2d_list(c, pairs, idx, K, d_dst);
    if (algo == ACX_ALGO_SIMPLE) return run_simple_list(c, pairs, idx, K, *static_cast<const acx_simple_params *>(params), d_dst);
    ScratchReserve reserve(c, reserve_bytes);
    DevDst dd{d_dst, idx};
    if (algo == ACX_ALGO_EARLYFUSION)
        return run_ef(c, pairs, K, *static_cast<const acx_ef_params *>(params), nullptr, nullptr, nullptr, 0, 0, &dd);
    return run_serra09(c, pairs, K, *static_cast<const acx_serra09_params *>(params), nullptr, nullptr, algo == ACX_ALGO_CHENFUSION, &dd);
}

int acx_grid_run(acx_ctx *c, const acx_grid_spec *spec, const void *params, int32_t rank, int64_t first, int64_t count,
                 float *d_scores)
{
    if (!c) return ACX_ERR_INVALID;
    if (!acx::grid_spec_ok(spec) || (!params && spec->algo != ACX_ALGO_FTM2D) || !d_scores || rank < 0 || rank >= spec->world || first < 0)
        return fail(c, ACX_ERR_INVALID, "grid_run: bad argument");
    std::vector<int64_t> len;
    int rc = pool_lengths(c, spec->algo, len);
    if (rc != ACX_OK) return rc;
    ACX_HIP(c, hipSetDevice(c->device));
    const std::vector<acx_grid_tile> mine = acx::grid_slice(cached_plan(c, len, *spec), rank, first, count);
    if (mine.empty()) return ACX_OK;
    const int w = acx::grid_planes(spec->algo);
    {   // blocks of one rank are contiguous in deal order: zero the slice (diagonal blocks keep zeros)
        const int64_t lo = mine.front().offset;
        const int64_t hi = mine.back().offset + (int64_t)mine.back().rows * mine.back().cols * w;
        ACX_HIP(c, hipMemsetAsync(d_scores + lo, 0, sizeof(float) * (size_t)(hi - lo), c->stream));
    }
    if (spec->algo == ACX_ALGO_FTM2D) {
        rc = run_ftm2d_tiles(c, mine, spec->symmetric, d_scores);
        if (rc != ACX_OK) return rc;
        ACX_HIP(c, hipStreamSynchronize(c->stream));
        return ACX_OK;
    }
    if (spec->algo == ACX_ALGO_SIMPLE) {
        if (!c->d_frames64) return fail(c, ACX_ERR_STATE, "grid_run: f64 feature pool not uploaded (acx_upload_pool_f64)");
        rc = run_simple_tiles(c, mine, spec->symmetric, *static_cast<const acx_simple_params *>(params), d_scores);
        if (rc != ACX_OK) return rc;
        ACX_HIP(c, hipStreamSynchronize(c->stream));
        drain_profile(c);
        return ACX_OK;
    }
    // Serra09 / ChenFusion / EarlyFusion: per-pair descriptors are built by the host (pairs of a few tiles at a
    // time); the scores go from the kernels' output straight into d_scores (scatter_scores_kernel)
    const int64_t CHUNK_PAIRS = (int64_t)1 << 20;
    std::vector<int32_t> pairs;
    std::vector<int64_t> idx;
    size_t t0 = 0;
    while (t0 < mine.size()) {
        pairs.clear(); idx.clear();
        size_t t1 = t0;
        while (t1 < mine.size() && (t1 == t0 || (int64_t)idx.size() + (int64_t)mine[t1].rows * mine[t1].cols <= CHUNK_PAIRS)) {
            acx::grid_tile_pairs(mine[t1], spec->symmetric, w, pairs, idx);
            ++t1;
        }
        if (!idx.empty() && (rc = run_pair_list(c, spec->algo, params, pairs.data(), idx.data(), (int64_t)idx.size(), d_scores, 0)) != ACX_OK)
            return rc;
        t0 = t1;
    }
    ACX_HIP(c, hipStreamSynchronize(c->stream));
    return ACX_OK;
}

int acx_grid_scatter(const int64_t *lengths, int32_t n_tracks, const acx_grid_spec *spec, const float *gathered,
                     int64_t rank_stride, int64_t first, int64_t count, float *const *D, int64_t ld, int32_t mirror)
{
    if (!lengths || n_tracks < 1 || !acx::grid_spec_ok(spec) || !gathered || !D || ld < n_tracks || first < 0) return ACX_ERR_INVALID;
    for (int e = 0; e < acx::grid_planes(spec->algo); ++e) if (!D[e]) return ACX_ERR_INVALID;
    std::vector<acx_grid_tile> tiles;
    std::vector<int64_t> fl;
    std::vector<double> co;
    acx::grid_plan(lengths, n_tracks, *spec, tiles, fl, co);
    for (int r = 0; r < spec->world; ++r) if (fl[r] > rank_stride) return ACX_ERR_INVALID;
    acx::grid_scatter(tiles, *spec, gathered, rank_stride, first, count, D, ld, mirror);
    return ACX_OK;
}

int acx_pair_grid(acx_ctx *c, const acx_grid_spec *spec, const void *params, float *const *D, int64_t ld, int32_t mirror)
{
    if (!c) return ACX_ERR_INVALID;
    if (!acx::grid_spec_ok(spec) || spec->world != 1 || (!params && spec->algo != ACX_ALGO_FTM2D) || !D)
        return fail(c, ACX_ERR_INVALID, "pair_grid: bad argument (world must be 1)");
    for (int e = 0; e < acx::grid_planes(spec->algo); ++e) if (!D[e]) return fail(c, ACX_ERR_INVALID, "pair_grid: null plane");
    std::vector<int64_t> len;
    int rc = pool_lengths(c, spec->algo, len);
    if (rc != ACX_OK) return rc;
    if (ld < (int64_t)len.size()) return fail(c, ACX_ERR_INVALID, "pair_grid: leading dimension smaller than the number of tracks");
    ACX_HIP(c, hipSetDevice(c->device));
    // slices of consecutive tiles (deal order) of at most SLICE floats: run on the device, one D2H copy of the
    // slice into pinned memory, scattered into the caller's planes -- the host never holds more than a slice
    const std::vector<acx_grid_tile> tiles = cached_plan(c, len, *spec);       // (a copy: grid_run re-reads the cache)
    const int w = acx::grid_planes(spec->algo);
    const int64_t SLICE = (int64_t)1 << 26;                                    // 256 MB of scores
    int64_t cap = 0;
    for (size_t a = 0; a < tiles.size();) {
        int64_t fl = 0;
        size_t b = a;
        while (b < tiles.size() && (b == a || fl + (int64_t)tiles[b].rows * tiles[b].cols * w <= SLICE)) { fl += (int64_t)tiles[b].rows * tiles[b].cols * w; ++b; }
        cap = std::max(cap, fl);
        a = b;
    }
    DeviceBuffer<float> d;
    PinnedBuffer<float> h;
    ACX_HIP(c, d.grow((size_t)std::max<int64_t>(1, cap)));
    if (h.grow((size_t)std::max<int64_t>(1, cap)) != hipSuccess) return fail(c, ACX_ERR_NOMEM, "pair_grid: cannot allocate the pinned staging slice");
    // development aid (ACX_GRID_TIMING=1): the host's seconds in the three steps of a slice
    static const bool grid_timing = [] { const char *e = getenv("ACX_GRID_TIMING"); return e && e[0] == '1'; }();
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double tg[3] = {0, 0, 0};
    int nslices = 0;
    for (size_t a = 0; a < tiles.size() && rc == ACX_OK;) {
        int64_t fl = 0;
        size_t b = a;
        while (b < tiles.size() && (b == a || fl + (int64_t)tiles[b].rows * tiles[b].cols * w <= SLICE)) { fl += (int64_t)tiles[b].rows * tiles[b].cols * w; ++b; }
        // grid_run writes tile t at d_scores + t.offset: rebase so that the slice starts at d[0]
        const double t_0 = now();
        rc = acx_grid_run(c, spec, params, 0, (int64_t)a, (int64_t)(b - a), d - tiles[a].offset);
        const double t_1 = now();
        if (rc == ACX_OK) {
            const hipError_t e = hipMemcpy(h, d, sizeof(float) * (size_t)fl, hipMemcpyDeviceToHost);
            if (e != hipSuccess) rc = fail(c, ACX_ERR_HIP, std::string("pair_grid: ") + hipGetErrorString(e));
        }
        const double t_2 = now();
        if (rc == ACX_OK) {
            std::vector<acx_grid_tile> part(tiles.begin() + a, tiles.begin() + b);
            for (acx_grid_tile &t : part) t.offset -= tiles[a].offset;
            acx::grid_scatter(part, *spec, h, 0, 0, -1, D, ld, mirror);
        }
        tg[0] += t_1 - t_0; tg[1] += t_2 - t_1; tg[2] += now() - t_2;
        ++nslices;
        a = b;
    }
    if (grid_timing)
        fprintf(stderr, "[acx pair_grid] %d slice(s): device %.2f s, copy to the host %.2f s, scatter + mirror %.2f s\n", nslices, tg[0], tg[1], tg[2]);
    return rc;
}

// ---------------------------------------------------------------------------------------
// Query bands: given queries against the uploaded collection, scores / top-k without an N x N matrix
// ---------------------------------------------------------------------------------------
// A band is R query rows x N columns x planes floats on the device (the slab, plane fastest), filled by the pair
// kernels through a DevDst and finished by query_kernels.hpp.  A band's device memory -- slab plus its results -- takes
// at most HALF of the scratch limit; while the pair kernels of a band run under a limit the caller set, they see what
// is left of it.  Which pairs a band holds, its rows and the layout of a call's device block: query_plan.hpp.
struct QueryCall {
    int algo = 0, w = 1, n = 0, symmetric = 0, mode = 0;
    const void *params = nullptr;
};

// Everything both calls check of their common arguments, before anything is allocated or launched.
static int query_check(acx_ctx *c, const char *who, const acx_query_spec *spec, const void *params, const int32_t *queries,
                       int32_t n_queries, const int32_t *cands, int32_t n_cands, const double *col, QueryCall &Q)
{
    const std::string w(who);
    if (!spec) return fail(c, ACX_ERR_INVALID, w + ": spec must not be NULL");
    if (acx::grid_planes(spec->algo) <= 0) return fail(c, ACX_ERR_INVALID, w + ": spec.algo = " + std::to_string(spec->algo) + " is not an ACX_ALGO_* value");
    if (spec->symmetric != 0 && spec->symmetric != 1) return fail(c, ACX_ERR_INVALID, w + ": spec.symmetric must be 0 or 1");
    if (spec->col_mode < 0 || spec->col_mode > 2) return fail(c, ACX_ERR_INVALID, w + ": spec.col_mode must be 0, 1 or 2");
    if (spec->reserved != 0) return fail(c, ACX_ERR_INVALID, w + ": spec.reserved must be 0");
    if (!params && spec->algo != ACX_ALGO_FTM2D) return fail(c, ACX_ERR_INVALID, w + ": params must not be NULL for this algorithm");
    std::vector<int64_t> len;
    const int rc = pool_lengths(c, spec->algo, len);
    if (rc != ACX_OK) return fail(c, rc, w + ": the pool of spec.algo is not uploaded (" + c->err + ")");
    const int n = (int)len.size();
    if (n_queries < 0) return fail(c, ACX_ERR_INVALID, w + ": n_queries must be >= 0 (got " + std::to_string(n_queries) + ")");
    if (n_queries > 0 && !queries) return fail(c, ACX_ERR_INVALID, w + ": queries must not be NULL");
    for (int32_t i = 0; i < n_queries; ++i)
        if (queries[i] < 0 || queries[i] >= n)
            return fail(c, ACX_ERR_INVALID, w + ": queries[" + std::to_string(i) + "] = " + std::to_string(queries[i]) + " is not a track in [0, " + std::to_string(n) + ")");
    if (cands) {
        if (n_cands < 0) return fail(c, ACX_ERR_INVALID, w + ": n_cands must be >= 0 (got " + std::to_string(n_cands) + ")");
        for (int32_t j = 0; j < n_cands; ++j) {
            if (cands[j] < 0 || cands[j] >= n)
                return fail(c, ACX_ERR_INVALID, w + ": cands[" + std::to_string(j) + "] = " + std::to_string(cands[j]) + " is not a track in [0, " + std::to_string(n) + ")");
            if (j > 0 && cands[j] <= cands[j - 1])
                return fail(c, ACX_ERR_INVALID, w + ": cands must be strictly ascending (cands[" + std::to_string(j) + "])");
        }
    }
    if (spec->col_mode == 0 && col) return fail(c, ACX_ERR_INVALID, w + ": col must be NULL when spec.col_mode is 0");
    if (spec->col_mode != 0 && !col) return fail(c, ACX_ERR_INVALID, w + ": col must not be NULL when spec.col_mode is 1 or 2");
    if (col)
        for (int i = 0; i < n; ++i)
            if (!std::isfinite(col[i])) return fail(c, ACX_ERR_INVALID, w + ": col[" + std::to_string(i) + "] is not finite");
    Q.algo = spec->algo; Q.w = acx::grid_planes(spec->algo); Q.n = n; Q.symmetric = spec->symmetric; Q.mode = spec->col_mode;
    Q.params = params;
    return ACX_OK;
}

// Rows per band: `per_row` bytes of device memory per query row within half of the scratch limit, `cap` rows at most.
static int query_band_rows(acx_ctx *c, const char *who, int n_queries, int64_t per_row, int64_t cap, int *rows)
{
    *rows = acx::query_band_rows(n_queries, per_row, scratch_limit_bytes(c) / 2, cap);
    if (*rows > 0) return ACX_OK;
    return fail(c, ACX_ERR_NOMEM, std::string(who) + ": one query row (" + std::to_string(per_row) + " bytes of scores and results) does not fit half of the scratch limit");
}

extern "C++" {
// Part `at` of a call's block as an array of T.  `src` is on its way there; NULL: the call has no such part, d is null.
template <typename T>
static int query_part(acx_ctx *c, char *d_mem, size_t at, const T *src, size_t count, const T *&d)
{
    d = src ? reinterpret_cast<const T *>(d_mem + at) : nullptr;
    if (src && count > 0) ACX_HIP(c, hipMemcpyAsync(d_mem + at, src, sizeof(T) * count, hipMemcpyHostToDevice, c->stream));
    return ACX_OK;
}
template <typename T> static T *query_out(char *d_mem, size_t at) { return reinterpret_cast<T *>(d_mem + at); }
}  // extern "C++"

// The head of every call's block: the slab, the column values (null without) and the queries, both on their way there.
struct QueryHeadDev { float *slab; const double *col; const int32_t *q; };

static int query_upload_head(acx_ctx *c, char *d_mem, const acx::QueryHead &h, const double *col, int n, const int32_t *queries, int n_queries,
                             QueryHeadDev &d)
{
    d.slab = query_out<float>(d_mem, h.slab);
    const int rc = query_part(c, d_mem, h.col, col, (size_t)n, d.col);
    return rc != ACX_OK ? rc : query_part(c, d_mem, h.queries, queries, (size_t)n_queries, d.q);
}

// One band through the pair kernels: rows queries[r0 .. r0 + nr) against the columns (`list`: ncols of them, NULL: all
// of 0 .. ncols).  On return every score of the band lies in d_slab.  FTM2D takes the tile kernel (query_plan.hpp).
static int query_run_band(acx_ctx *c, const QueryCall &Q, const int32_t *queries, int r0, int nr, const int32_t *cols, int ncols, float *d_slab,
                          int64_t band_bytes, std::vector<int32_t> &pairs, std::vector<int64_t> &idx)
{
    ACX_HIP(c, hipMemsetAsync(d_slab, 0, sizeof(float) * (size_t)nr * Q.n * Q.w, c->stream));
    int rc = ACX_OK;
    if (Q.algo == ACX_ALGO_FTM2D) {
        ProfScope ps(c, KS_FTMTILE, (int64_t)nr * ncols);
        rc = run_ftm2d_tiles(c, acx::query_ftm2d_band_tiles(queries + r0, nr, cols, ncols, Q.n, Q.symmetric), Q.symmetric, d_slab);
    } else {
        acx::query_band_pairs(queries + r0, nr, cols, ncols, Q.n, Q.w, Q.symmetric, pairs, idx);
        // a limit the caller set covers the band too: the pair kernels batch within what the band leaves of it
        if (!idx.empty()) rc = run_pair_list(c, Q.algo, Q.params, pairs.data(), idx.data(), (int64_t)idx.size(), d_slab, band_bytes);
    }
    if (rc != ACX_OK) return rc;
    ACX_HIP(c, hipStreamSynchronize(c->stream));
    return ACX_OK;
}

// One list band -- every query brings its own candidate list (acx_query_topk_lists): R query rows x L list positions x
// planes floats (slab[(r L + j) W + e]), only the listed cells exist.  On return every listed cell's score lies in d_slab.
static int query_run_list_band(acx_ctx *c, const QueryCall &Q, const int32_t *queries, int r0, int nr, const int32_t *lists, int L, float *d_slab,
                               int64_t band_bytes, std::vector<int32_t> &pairs, std::vector<int64_t> &idx)
{
    if (L > 0) ACX_HIP(c, hipMemsetAsync(d_slab, 0, sizeof(float) * (size_t)nr * L * Q.w, c->stream));
    acx::query_list_pairs(queries + r0, nr, lists + (size_t)r0 * L, L, Q.w, Q.symmetric, pairs, idx);
    if (!idx.empty()) {
        const int rc = run_pair_list(c, Q.algo, Q.params, pairs.data(), idx.data(), (int64_t)idx.size(), d_slab, band_bytes);
        if (rc != ACX_OK) return rc;
    }
    ACX_HIP(c, hipStreamSynchronize(c->stream));
    return ACX_OK;
}

typedef int (*QueryBandFill)(acx_ctx *, const QueryCall &, const int32_t *, int, int, const int32_t *, int, float *, int64_t, std::vector<int32_t> &,
                             std::vector<int64_t> &);

// The bands of a call, R query rows each: fill (query_run_band or query_run_list_band, with the call's `list` and `len`)
// brings the band's scores into d_slab, then launch(r0, nr) -- the call's finishing kernel -- and, the launches checked,
// copies(r0, nr) -- its results on their way to the host.
extern "C++" {
template <typename L, typename C>
static int query_for_bands(acx_ctx *c, const QueryCall &Q, const int32_t *queries, int n_queries, int R, QueryBandFill fill, const int32_t *list,
                           int len, float *d_slab, int64_t per_row, L launch, C copies)
{
    std::vector<int32_t> pairs;
    std::vector<int64_t> idx;
    for (int r0 = 0; r0 < n_queries; r0 += R) {
        const int nr = std::min(R, n_queries - r0);
        int rc = fill(c, Q, queries, r0, nr, list, len, d_slab, (int64_t)R * per_row, pairs, idx);
        if (rc != ACX_OK) return rc;
        launch(r0, nr);
        ACX_LAUNCHES_OK(c);
        if ((rc = copies(r0, nr)) != ACX_OK) return rc;
        ACX_HIP(c, hipStreamSynchronize(c->stream));
    }
    return ACX_OK;
}
}  // extern "C++"

// The results of a top-k band on their way to the host (acx_query_topk, acx_query_topk_lists)
static int query_topk_copies(acx_ctx *c, int r0, int nr, int w, int k, const int32_t *d_idx, const float *d_sc, int32_t *out_idx, float *out_score)
{
    const size_t nres = (size_t)nr * w * k;
    ACX_HIP(c, hipMemcpyAsync(out_idx + (size_t)r0 * w * k, d_idx, 4 * nres, hipMemcpyDeviceToHost, c->stream));
    ACX_HIP(c, hipMemcpyAsync(out_score + (size_t)r0 * w * k, d_sc, 4 * nres, hipMemcpyDeviceToHost, c->stream));
    return ACX_OK;
}

int acx_query_scores(acx_ctx *c, const acx_query_spec *spec, const void *params, const int32_t *queries, int32_t n_queries,
                     const double *col, float *const *rows, int64_t ld)
{
    if (!c) return ACX_ERR_INVALID;
    QueryCall Q;
    int rc = query_check(c, "query_scores", spec, params, queries, n_queries, nullptr, 0, col, Q);
    if (rc != ACX_OK) return rc;
    if (!rows) return fail(c, ACX_ERR_INVALID, "query_scores: rows must not be NULL");
    for (int e = 0; e < Q.w; ++e)
        if (n_queries > 0 && !rows[e]) return fail(c, ACX_ERR_INVALID, "query_scores: rows[" + std::to_string(e) + "] must not be NULL");
    if (ld < Q.n) return fail(c, ACX_ERR_INVALID, "query_scores: ld = " + std::to_string(ld) + " is smaller than the number of tracks " + std::to_string(Q.n));
    if (n_queries == 0) return ACX_OK;
    const int64_t per_row = 2 * (int64_t)Q.n * Q.w * 4;           // the slab row and its finished copy
    int R = 0;
    if ((rc = query_band_rows(c, "query_scores", n_queries, per_row, acx::QUERY_BAND_ROWS, &R)) != ACX_OK) return rc;
    ACX_HIP(c, hipSetDevice(c->device));
    const acx::QueryScoresLayout lay = acx::query_scores_layout((size_t)R * Q.n * Q.w, col ? Q.n : 0, n_queries);
    return with_device_block(c, "query_scores", lay.total, [&](char *d_mem) -> int {
        QueryHeadDev d;
        const int rc2 = query_upload_head(c, d_mem, lay.head, col, Q.n, queries, n_queries, d);
        if (rc2 != ACX_OK) return rc2;
        float *d_fin = query_out<float>(d_mem, lay.fin);
        return query_for_bands(c, Q, queries, n_queries, R, query_run_band, nullptr, Q.n, d.slab, per_row,
            [&](int r0, int nr) {
                ProfScope ps(c, KS_QROWS, (int64_t)nr * Q.n * Q.w);
                hipLaunchKernelGGL(acx::query_rows_kernel, dim3((unsigned)((Q.n + 255) / 256), (unsigned)nr, (unsigned)Q.w), dim3(256), 0, c->stream,
                                   d.slab, Q.n, Q.w, nr, d.q + r0, d.col, Q.mode, d_fin);
            },
            [&](int r0, int nr) -> int {
                for (int e = 0; e < Q.w; ++e)
                    ACX_HIP(c, hipMemcpy2DAsync(rows[e] + (size_t)r0 * ld, sizeof(float) * (size_t)ld, d_fin + (size_t)e * nr * Q.n, sizeof(float) * (size_t)Q.n,
                                                sizeof(float) * (size_t)Q.n, (size_t)nr, hipMemcpyDeviceToHost, c->stream));
                return ACX_OK;
            });
    });
}

int acx_query_topk(acx_ctx *c, const acx_query_spec *spec, const void *params, const int32_t *queries, int32_t n_queries,
                   const int32_t *cands, int32_t n_cands, const double *col, int32_t k, int32_t *out_idx, float *out_score)
{
    if (!c) return ACX_ERR_INVALID;
    QueryCall Q;
    int rc = query_check(c, "query_topk", spec, params, queries, n_queries, cands, n_cands, col, Q);
    if (rc != ACX_OK) return rc;
    if ((rc = rank_check_k(c, "query_topk", k, n_queries, out_idx, out_score)) != ACX_OK) return rc;
    if (n_queries == 0) return ACX_OK;
    const int ncand = cands ? n_cands : Q.n;
    const int64_t per_row = (int64_t)Q.n * Q.w * 4 + 8 * (int64_t)Q.w * k;      // the slab row and its results
    int R = 0;
    if ((rc = query_band_rows(c, "query_topk", n_queries, per_row, acx::QUERY_BAND_ROWS, &R)) != ACX_OK) return rc;
    ACX_HIP(c, hipSetDevice(c->device));
    if (!c->query_attr) {
        ACX_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(acx::query_topk_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       4 * acx::RANK_ROW_LDS + 12 * acx::RANK_KMAX + acx::RANK_SELECT_LDS_FIXED));
        c->query_attr = true;
    }
    int P = 4;
    while (P < std::min<int>(k, ncand)) P <<= 1;
    const acx::QueryTopkLayout lay = acx::query_topk_layout((size_t)R * Q.n * Q.w, col ? Q.n : 0, n_queries, cands ? n_cands : 0, (size_t)R * Q.w * k);
    return with_device_block(c, "query_topk", lay.total, [&](char *d_mem) -> int {
        QueryHeadDev d;
        const int32_t *d_c;
        int rc2 = query_upload_head(c, d_mem, lay.head, col, Q.n, queries, n_queries, d);
        if (rc2 != ACX_OK || (rc2 = query_part(c, d_mem, lay.list, cands, (size_t)n_cands, d_c)) != ACX_OK) return rc2;
        int32_t *d_idx = query_out<int32_t>(d_mem, lay.idx);
        float *d_sc = query_out<float>(d_mem, lay.score);
        const bool in_lds = ncand <= acx::RANK_ROW_LDS;
        const size_t lds = 12 * (size_t)P + acx::RANK_SELECT_LDS_FIXED + (in_lds ? 4 * (size_t)ncand : 0);
        return query_for_bands(c, Q, queries, n_queries, R, query_run_band, cands, ncand, d.slab, per_row,
            [&](int r0, int nr) {
                ProfScope ps(c, KS_QTOPK, (int64_t)nr * ncand * Q.w);
                ACX_LAUNCH_IN_LDS(query_topk_kernel, in_lds, dim3((unsigned)nr, (unsigned)Q.w), lds, d.slab, Q.n, Q.w, d.q + r0, d_c, ncand, d.col, Q.mode,
                                  (int)k, P, d_idx, d_sc);
            },
            [&](int r0, int nr) { return query_topk_copies(c, r0, nr, Q.w, k, d_idx, d_sc, out_idx, out_score); });
    });
}

int acx_query_ranks(acx_ctx *c, const acx_query_spec *spec, const void *params, const int32_t *queries, int32_t n_queries,
                    const double *col, const int32_t *posn, const int64_t *moff, const int32_t *mates, int32_t *out_pos,
                    uint8_t *out_flag)
{
    if (!c) return ACX_ERR_INVALID;
    QueryCall Q;
    int rc = query_check(c, "query_ranks", spec, params, queries, n_queries, nullptr, 0, col, Q);
    if (rc != ACX_OK) return rc;
    if ((rc = rank_check_mates(c, "query_ranks", Q.n, n_queries, queries, "track", "is queries[", "] itself", moff, mates, out_pos, out_flag)) != ACX_OK)
        return rc;
    const int64_t M = moff[n_queries];
    int64_t maxm = 0;
    for (int32_t r = 0; r < n_queries; ++r) maxm = std::max(maxm, moff[r + 1] - moff[r]);
    if (posn) {
        std::vector<std::pair<int32_t, int32_t>> seen((size_t)Q.n);
        for (int i = 0; i < Q.n; ++i) {
            if (posn[i] < 0) return fail(c, ACX_ERR_INVALID, "query_ranks: posn[" + std::to_string(i) + "] = " + std::to_string(posn[i]) + " is negative");
            seen[i] = {posn[i], i};
        }
        std::sort(seen.begin(), seen.end());
        for (int i = 1; i < Q.n; ++i)
            if (seen[i].first == seen[i - 1].first)
                return fail(c, ACX_ERR_INVALID, "query_ranks: posn must hold distinct tie ranks (posn[" + std::to_string(seen[i].second) + "] = posn[" +
                                                    std::to_string(seen[i - 1].second) + "] = " + std::to_string(seen[i].first) + ")");
    }
    if (n_queries == 0) return ACX_OK;
    // the slab row and its results: every row is charged the longest mate list of the call (positions and flags per plane)
    const int64_t per_row = (int64_t)Q.n * Q.w * 4 + (int64_t)Q.w * (4 * maxm + 1);
    int R = 0;
    if ((rc = query_band_rows(c, "query_ranks", n_queries, per_row, acx::QUERY_BAND_ROWS, &R)) != ACX_OK) return rc;
    ACX_HIP(c, hipSetDevice(c->device));
    if (!c->query_rank_attr) {
        ACX_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(acx::query_rank_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       4 * acx::RANK_ROW_LDS + acx::RANK_COUNT_LDS_FIXED));
        c->query_rank_attr = true;
    }
    int64_t band_m = 0;                                // the most positions one band returns per plane
    for (int r0 = 0; r0 < n_queries; r0 += R) band_m = std::max(band_m, moff[std::min(n_queries, r0 + R)] - moff[r0]);
    const acx::QueryRanksLayout lay = acx::query_ranks_layout((size_t)R * Q.n * Q.w, col ? Q.n : 0, n_queries, (size_t)M, posn ? Q.n : 0,
                                                              (size_t)Q.w * (size_t)band_m, (size_t)R * Q.w);
    return with_device_block(c, "query_ranks", lay.total, [&](char *d_mem) -> int {
        QueryHeadDev d;
        const int64_t *d_moff;
        const int32_t *d_mates, *d_posn;
        int rc2 = query_upload_head(c, d_mem, lay.head, col, Q.n, queries, n_queries, d);
        if (rc2 != ACX_OK || (rc2 = query_part(c, d_mem, lay.moff, moff, (size_t)n_queries + 1, d_moff)) != ACX_OK ||
            (rc2 = query_part(c, d_mem, lay.mates, mates, (size_t)M, d_mates)) != ACX_OK ||
            (rc2 = query_part(c, d_mem, lay.posn, posn, (size_t)Q.n, d_posn)) != ACX_OK)
            return rc2;
        int32_t *d_pos = query_out<int32_t>(d_mem, lay.pos);
        uint8_t *d_flag = query_out<uint8_t>(d_mem, lay.flag);
        const bool in_lds = Q.n <= acx::RANK_ROW_LDS;
        const size_t lds = acx::RANK_COUNT_LDS_FIXED + (in_lds ? 16 * (size_t)((Q.n + 3) / 4) : 0);
        // (a band's positions per plane: moff[r0 + nr] - moff[r0])
        return query_for_bands(c, Q, queries, n_queries, R, query_run_band, nullptr, Q.n, d.slab, per_row,
            [&](int r0, int nr) {
                ProfScope ps(c, KS_QRANK, (int64_t)nr * Q.n * Q.w);
                ACX_LAUNCH_IN_LDS(query_rank_kernel, in_lds, dim3((unsigned)nr, (unsigned)Q.w), lds, d.slab, Q.n, Q.w, d.q + r0, d.col, Q.mode, d_posn,
                                  d_moff + r0, d_mates + moff[r0], moff[r0], moff[r0 + nr] - moff[r0], d_pos, d_flag);
            },
            [&](int r0, int nr) -> int {
                const int64_t mb = moff[r0 + nr] - moff[r0];
                for (int e = 0; e < Q.w && mb > 0; ++e)
                    ACX_HIP(c, hipMemcpyAsync(out_pos + (size_t)e * M + moff[r0], d_pos + (size_t)e * mb, 4 * (size_t)mb, hipMemcpyDeviceToHost, c->stream));
                ACX_HIP(c, hipMemcpyAsync(out_flag + (size_t)r0 * Q.w, d_flag, (size_t)nr * Q.w, hipMemcpyDeviceToHost, c->stream));
                return ACX_OK;
            });
    });
}

// Everything acx_query_topk_lists checks of its lists, before anything is allocated or launched.
static int query_check_lists(acx_ctx *c, const char *who, int n, int32_t n_queries, const int32_t *lists, int32_t list_len)
{
    const std::string w(who);
    if (list_len < 0) return fail(c, ACX_ERR_INVALID, w + ": list_len must be >= 0 (got " + std::to_string(list_len) + ")");
    if (n_queries > 0 && list_len > 0 && !lists) return fail(c, ACX_ERR_INVALID, w + ": lists must not be NULL when list_len > 0");
    std::vector<std::pair<int32_t, int32_t>> seen;
    for (int32_t i = 0; i < n_queries; ++i) {
        const int32_t *row = lists + (size_t)i * list_len;
        seen.clear();
        for (int32_t j = 0; j < list_len; ++j) {
            if (row[j] < -1 || row[j] >= n)
                return fail(c, ACX_ERR_INVALID, w + ": lists[" + std::to_string(i) + "][" + std::to_string(j) + "] = " + std::to_string(row[j]) +
                                                    " is neither a track in [0, " + std::to_string(n) + ") nor -1");
            if (row[j] >= 0) seen.push_back({row[j], j});
        }
        std::sort(seen.begin(), seen.end());
        for (size_t s = 1; s < seen.size(); ++s)
            if (seen[s].first == seen[s - 1].first)
                return fail(c, ACX_ERR_INVALID, w + ": lists row " + std::to_string(i) + " holds track " + std::to_string(seen[s].first) +
                                                    " twice (positions " + std::to_string(seen[s - 1].second) + " and " + std::to_string(seen[s].second) + ")");
    }
    return ACX_OK;
}

int acx_query_topk_lists(acx_ctx *c, const acx_query_spec *spec, const void *params, const int32_t *queries, int32_t n_queries,
                         const int32_t *lists, int32_t list_len, const double *col, int32_t k, int32_t *out_idx, float *out_score)
{
    if (!c) return ACX_ERR_INVALID;
    QueryCall Q;
    int rc = query_check(c, "query_topk_lists", spec, params, queries, n_queries, nullptr, 0, col, Q);
    if (rc != ACX_OK) return rc;
    if ((rc = rank_check_k(c, "query_topk_lists", k, n_queries, out_idx, out_score)) != ACX_OK) return rc;
    if ((rc = query_check_lists(c, "query_topk_lists", Q.n, n_queries, lists, list_len)) != ACX_OK) return rc;
    if (n_queries == 0) return ACX_OK;
    const int L = list_len;
    const int64_t per_row = (int64_t)L * Q.w * 4 + 8 * (int64_t)Q.w * k;        // the slab row and its results
    int R = 0;                                                                  // (bounded by cells, not by rows: query_plan.hpp)
    if ((rc = query_band_rows(c, "query_topk_lists", n_queries, per_row, acx::query_list_band_cap(L), &R)) != ACX_OK) return rc;
    ACX_HIP(c, hipSetDevice(c->device));
    if (!c->query_lists_attr) {
        ACX_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(acx::query_topk_lists_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       4 * acx::RANK_ROW_LDS + 12 * acx::RANK_KMAX + acx::RANK_SELECT_LDS_FIXED + 16));
        c->query_lists_attr = true;
    }
    int P = 4;
    while (P < std::min<int>(k, L)) P <<= 1;
    const acx::QueryTopkLayout lay = acx::query_topk_layout((size_t)R * L * Q.w, col ? Q.n : 0, n_queries, (size_t)n_queries * L, (size_t)R * Q.w * k);
    return with_device_block(c, "query_topk_lists", lay.total, [&](char *d_mem) -> int {
        QueryHeadDev d;
        const int32_t *d_l;
        int rc2 = query_upload_head(c, d_mem, lay.head, col, Q.n, queries, n_queries, d);
        if (rc2 != ACX_OK || (rc2 = query_part(c, d_mem, lay.list, lists, (size_t)n_queries * L, d_l)) != ACX_OK) return rc2;
        int32_t *d_idx = query_out<int32_t>(d_mem, lay.idx);
        float *d_sc = query_out<float>(d_mem, lay.score);
        const bool in_lds = L <= acx::RANK_ROW_LDS;
        const size_t lds = 12 * (size_t)P + acx::RANK_SELECT_LDS_FIXED + 16 + (in_lds ? 4 * (size_t)L : 0);
        return query_for_bands(c, Q, queries, n_queries, R, query_run_list_band, lists, L, d.slab, per_row,
            [&](int r0, int nr) {
                ProfScope ps(c, KS_QTOPKL, (int64_t)nr * L * Q.w);
                ACX_LAUNCH_IN_LDS(query_topk_lists_kernel, in_lds, dim3((unsigned)nr, (unsigned)Q.w), lds, d.slab, L, Q.w, d.q + r0, d_l + (size_t)r0 * L,
                                  d.col, Q.mode, (int)k, P, d_idx, d_sc);
            },
            [&](int r0, int nr) { return query_topk_copies(c, r0, nr, Q.w, k, d_idx, d_sc, out_idx, out_score); });
    });
}

// ---- fused scores for query shortlists: Q small similarity network fusions side by side (snf_batch_kernels.hpp) ------
// What acx_query_fused_lists checks of its struct, before anything is allocated or launched.
static int fused_check_spec(acx_ctx *c, const char *who, const acx_fused_spec *f, int W, int col_mode)
{
    const std::string w(who);
    if (!f) return fail(c, ACX_ERR_INVALID, w + ": fused must not be NULL");
    if (f->reserved != 0) return fail(c, ACX_ERR_INVALID, w + ": fused.reserved must be 0");
    if (f->n_types < 1 || f->n_types > acx::FUSED_MAX_TYPES) return fail(c, ACX_ERR_INVALID, w + ": fused.n_types must be 1 or 2 (got " + std::to_string(f->n_types) + ")");
    for (int t = 0; t < f->n_types; ++t) {
        if (f->count[t] < 2 || f->count[t] > acx::FUSED_MAX_PLANES)
            return fail(c, ACX_ERR_INVALID, w + ": fused.count[" + std::to_string(t) + "] must be in 2..4 (got " + std::to_string(f->count[t]) + ")");
        for (int i = 0; i < f->count[t]; ++i)
            if (f->planes[t][i] < 0 || f->planes[t][i] >= W)
                return fail(c, ACX_ERR_INVALID, w + ": fused.planes[" + std::to_string(t) + "][" + std::to_string(i) + "] = " + std::to_string(f->planes[t][i]) +
                                                    " is not a plane in [0, " + std::to_string(W) + ")");
    }
    if (f->transform != ACX_FUSED_SQRTLEN && f->transform != ACX_FUSED_INV1P) return fail(c, ACX_ERR_INVALID, w + ": fused.transform is not an ACX_FUSED_* value");
    if (col_mode != (f->transform == ACX_FUSED_SQRTLEN ? 2 : 0))
        return fail(c, ACX_ERR_INVALID, w + ": spec.col_mode must be 2 with ACX_FUSED_SQRTLEN and 0 with ACX_FUSED_INV1P");
    if (f->K < 1) return fail(c, ACX_ERR_INVALID, w + ": fused.K must be >= 1 (got " + std::to_string(f->K) + ")");
    if (f->K > acx::FUSED_MAX_K) return fail(c, ACX_ERR_UNSUPPORTED, w + ": more than 64 neighbours are not supported on the device (fused.K = " + std::to_string(f->K) + ")");
    if (f->niters < 1) return fail(c, ACX_ERR_INVALID, w + ": fused.niters must be >= 1 (got " + std::to_string(f->niters) + ")");
    if (!(f->mu > 0.0)) return fail(c, ACX_ERR_INVALID, w + ": fused.mu must be > 0");
    if (!std::isfinite(f->reg_diag)) return fail(c, ACX_ERR_INVALID, w + ": fused.reg_diag must be finite");
    return ACX_OK;
}

// The device side of a chunk, as its kernels take it
struct FusedDev {
    const acx::FusedProb *probs; const int32_t *tracks; double *mats; double *V; int32_t *J;
    int P, max_n, M;
};

// One fused type of a chunk, all problems at once, launch for launch the sequence of acx_snf_fuse_dists (snf_prepare_dev per
// matrix, snf_loop): the distances of the type's planes lie in the D slots; on return the fused matrices lie in the acc slots.
static void fused_snf_batch(acx_ctx *c, const FusedDev &d, int m, int K, int niters, double reg_diag, double mu)
{
    const int M = d.M, n = d.max_n;
    const unsigned P = (unsigned)d.P, cells = (unsigned)(((int64_t)n * n + 255) / 256), rows4 = (unsigned)((n + 3) / 4), t32 = (unsigned)((n + 31) / 32);
    const int acc = acx::fused_slot_acc(M), ut = acx::fused_slot_ut(M), md = acx::fused_slot_md(M);
    {
        ProfScope ps(c, KS_SNFBATCHPREP, (int64_t)d.P * m);
        for (int i = 0; i < m; ++i) {
            hipLaunchKernelGGL(acx::snf_batch_sym_kernel, dim3(t32, t32, P), dim3(256), 0, c->stream, d.probs, d.mats, acx::fused_slot_dist(M, i), ut);
            hipLaunchKernelGGL(acx::snf_batch_localscale_kernel, dim3(rows4, P), dim3(256), 0, c->stream, d.probs, d.mats, ut, md, K);
            hipLaunchKernelGGL(acx::snf_batch_affinity_kernel, dim3(cells, P), dim3(256), 0, c->stream, d.probs, d.mats, ut, md, mu);
            hipLaunchKernelGGL(acx::snf_batch_knn_kernel, dim3(rows4, P), dim3(256), 0, c->stream, d.probs, d.mats, ut, d.J, d.V, i, K);
            hipLaunchKernelGGL(acx::snf_batch_rownorm_kernel, dim3((unsigned)n, P), dim3(256), 0, c->stream, d.probs, d.mats, ut, acx::fused_slot_cur(M, i));
        }
    }
    ProfScope ps(c, KS_SNFBATCHUPDATE, (int64_t)d.P * m * niters);
    for (int it = 0; it < niters; ++it)
        for (int i = 0; i < m; ++i) {
            // (from the second sweep on the two work lists alias, as in snf_loop)
            acx::SnfSlots sp;
            sp.count = 0;
            for (int k = 0; k < m; ++k)
                if (k != i) sp.s[sp.count++] = it == 0 ? acx::fused_slot_cur(M, k) : acx::fused_slot_nxt(M, k);
            hipLaunchKernelGGL(acx::snf_batch_mean_kernel, dim3(cells, P), dim3(256), 0, c->stream, d.probs, d.mats, sp, 1.0 / (double)(m - 1), acc);
            hipLaunchKernelGGL(acx::snf_batch_ast_kernel, dim3((unsigned)n, P), dim3(256), (size_t)n * sizeof(double), c->stream, d.probs, d.mats, acc, ut,
                               d.J, d.V, i, K);
            hipLaunchKernelGGL(acx::snf_batch_sut_kernel, dim3((unsigned)n, P), dim3(256), 0, c->stream, d.probs, d.mats, ut, acx::fused_slot_nxt(M, i), d.J,
                               d.V, i, K, reg_diag);
        }
    acx::SnfSlots sp;
    sp.count = m;
    for (int k = 0; k < m; ++k) sp.s[k] = acx::fused_slot_nxt(M, k);
    hipLaunchKernelGGL(acx::snf_batch_mean_kernel, dim3(cells, P), dim3(256), 0, c->stream, d.probs, d.mats, sp, 1.0 / (double)m, acc);
}

int acx_query_fused_lists(acx_ctx *c, const acx_query_spec *spec, const void *params, const int32_t *queries, int32_t n_queries,
                          const int32_t *lists, int32_t list_len, const double *col, const acx_fused_spec *fused, int32_t k,
                          int32_t *out_idx, float *out_score, uint8_t *out_flag)
{
    if (!c) return ACX_ERR_INVALID;
    const char *who = "query_fused_lists";
    QueryCall Q;
    int rc = query_check(c, who, spec, params, queries, n_queries, nullptr, 0, col, Q);
    if (rc != ACX_OK) return rc;
    if (Q.algo != ACX_ALGO_CHENFUSION && Q.algo != ACX_ALGO_EARLYFUSION)
        return fail(c, ACX_ERR_INVALID, std::string(who) + ": spec.algo must be ACX_ALGO_CHENFUSION or ACX_ALGO_EARLYFUSION (the classes with a late fusion)");
    if (Q.symmetric != 1) return fail(c, ACX_ERR_INVALID, std::string(who) + ": spec.symmetric must be 1 (a pair is scored as (min, max) and mirrored)");
    if ((rc = fused_check_spec(c, who, fused, Q.w, Q.mode)) != ACX_OK) return rc;
    if ((rc = rank_check_k(c, who, k, n_queries, out_idx, out_score)) != ACX_OK) return rc;
    if (n_queries > 0 && !out_flag) return fail(c, ACX_ERR_INVALID, std::string(who) + ": out_flag must not be NULL");
    if (list_len > acx::FUSED_MAX_LIST)
        return fail(c, ACX_ERR_UNSUPPORTED, std::string(who) + ": list_len = " + std::to_string(list_len) + " is over the limit of " + std::to_string(acx::FUSED_MAX_LIST));
    if ((rc = query_check_lists(c, who, Q.n, n_queries, lists, list_len)) != ACX_OK) return rc;
    const int L = list_len, K = fused->K, nt = fused->n_types;
    std::vector<int32_t> ns((size_t)n_queries);
    for (int32_t i = 0; i < n_queries; ++i) {
        int n = 1;
        for (int j = 0; j < L; ++j) n += (lists[(size_t)i * L + j] >= 0 && lists[(size_t)i * L + j] != queries[i]) ? 1 : 0;
        if (n < K + 2)
            return fail(c, ACX_ERR_INVALID, std::string(who) + ": lists row " + std::to_string(i) + " gives a neighbourhood of " + std::to_string(n) +
                                                " tracks (the query included); the fusion needs at least K + 2 = " + std::to_string(K + 2));
        ns[i] = n;
    }
    if (n_queries == 0) return ACX_OK;
    int M = 0;
    for (int t = 0; t < nt; ++t) M = std::max(M, fused->count[t]);
    int unfit = -1;
    const std::vector<int> ends = acx::fused_chunks(ns, Q.w, M, K, nt, k, scratch_limit_bytes(c) / 2, &unfit);
    if (unfit >= 0)
        return fail(c, ACX_ERR_NOMEM, std::string(who) + ": the neighbourhood of lists row " + std::to_string(unfit) + " (" + std::to_string(ns[unfit]) + " tracks, " +
                                          std::to_string(acx::fused_problem_bytes(ns[unfit], Q.w, M, K, nt, k)) + " bytes) does not fit half of the scratch limit");
    // the block is sized for the largest chunk of each part
    std::vector<acx::FusedChunk> chunks;
    size_t mx_pairs = 0, mx_mat = 0, mx_list = 0, mx_probs = 0, mx_tracks = 0;
    int max_n = 0;
    for (size_t ci = 0, first = 0; ci < ends.size(); first = (size_t)ends[ci++]) {
        chunks.push_back(acx::fused_chunk(queries, lists, L, (int)first, ends[ci], M, K));
        const acx::FusedChunk &ch = chunks.back();
        mx_pairs = std::max(mx_pairs, (size_t)ch.pairs); mx_mat = std::max(mx_mat, (size_t)ch.mat); mx_list = std::max(mx_list, (size_t)ch.list);
        mx_probs = std::max(mx_probs, ch.probs.size()); mx_tracks = std::max(mx_tracks, ch.tracks.size());
        max_n = std::max(max_n, ch.max_n);
    }
    ACX_HIP(c, hipSetDevice(c->device));
    int P2 = 4;
    while (P2 < std::min<int>(k, max_n - 1)) P2 <<= 1;
    const size_t row_lds = 12 * (size_t)P2 + acx::RANK_SELECT_LDS_FIXED + 4 * (size_t)max_n;
    const acx::FusedLayout lay = acx::fused_layout(mx_pairs * Q.w, col ? Q.n : 0, mx_mat, mx_list, mx_probs, mx_tracks, mx_probs * nt * k, mx_probs * nt);
    return with_device_block(c, who, lay.total, [&](char *d_mem) -> int {
        const double *d_col;
        int rc2 = query_part(c, d_mem, lay.col, col, (size_t)Q.n, d_col);
        if (rc2 != ACX_OK) return rc2;
        float *d_slab = query_out<float>(d_mem, lay.slab);
        int32_t *d_idx = query_out<int32_t>(d_mem, lay.idx);
        float *d_sc = query_out<float>(d_mem, lay.score);
        uint8_t *d_flag = query_out<uint8_t>(d_mem, lay.flag);
        std::vector<int32_t> pairs;
        std::vector<int64_t> idx;
        int first = 0;
        for (size_t ci = 0; ci < chunks.size(); first = ends[ci++]) {
            const acx::FusedChunk &ch = chunks[ci];
            const int P = (int)ch.probs.size();
            FusedDev d;
            d.mats = query_out<double>(d_mem, lay.mat); d.V = query_out<double>(d_mem, lay.V); d.J = query_out<int32_t>(d_mem, lay.J);
            d.P = P; d.max_n = ch.max_n; d.M = M;
            if ((rc2 = query_part(c, d_mem, lay.probs, ch.probs.data(), ch.probs.size(), d.probs)) != ACX_OK ||
                (rc2 = query_part(c, d_mem, lay.tracks, ch.tracks.data(), ch.tracks.size(), d.tracks)) != ACX_OK)
                return rc2;
            ACX_HIP(c, hipMemsetAsync(d_slab, 0, sizeof(float) * (size_t)ch.pairs * Q.w, c->stream));
            ACX_HIP(c, hipMemsetAsync(d_flag, 0, (size_t)P * nt, c->stream));
            acx::fused_chunk_pairs(ch, Q.w, pairs, idx);
            // a limit the caller set covers the chunk too: the pair kernels batch within what the chunk leaves of it
            if ((rc2 = run_pair_list(c, Q.algo, Q.params, pairs.data(), idx.data(), (int64_t)idx.size(), d_slab, (int64_t)lay.total)) != ACX_OK) return rc2;
            const unsigned cells = (unsigned)(((int64_t)ch.max_n * ch.max_n + 255) / 256);
            for (int t = 0; t < nt; ++t) {
                acx::FusedPlanes pl;
                pl.count = fused->count[t];
                for (int i = 0; i < acx::FUSED_MAX_PLANES; ++i) pl.p[i] = i < pl.count ? fused->planes[t][i] : 0;
                {
                    ProfScope ps(c, KS_FUSEDSTAGE, (int64_t)ch.pairs * pl.count);
                    hipLaunchKernelGGL(acx::fused_stage_kernel, dim3(cells, (unsigned)P), dim3(256), 0, c->stream, d.probs, d_slab, Q.w, d_col, d.tracks, pl,
                                       (int)fused->transform, d.mats, d_flag + t, nt);
                }
                fused_snf_batch(c, d, pl.count, K, fused->niters, fused->reg_diag, fused->mu);
                ProfScope ps(c, KS_FUSEDROW, (int64_t)P);
                hipLaunchKernelGGL(acx::fused_row_kernel, dim3((unsigned)P), dim3(acx::RANK_THREADS), row_lds, c->stream, d.probs, d.mats, acx::fused_slot_acc(M),
                                   d.tracks, (int)k, P2, d_idx, d_sc, nt * (int)k, t * (int)k);
            }
            ACX_LAUNCHES_OK(c);
            const size_t nres = (size_t)P * nt * k;
            ACX_HIP(c, hipMemcpyAsync(out_idx + (size_t)first * nt * k, d_idx, 4 * nres, hipMemcpyDeviceToHost, c->stream));
            ACX_HIP(c, hipMemcpyAsync(out_score + (size_t)first * nt * k, d_sc, 4 * nres, hipMemcpyDeviceToHost, c->stream));
            ACX_HIP(c, hipMemcpyAsync(out_flag + (size_t)first * nt, d_flag, (size_t)P * nt, hipMemcpyDeviceToHost, c->stream));
            // (the host vectors of the chunk and the descriptors' place in the block are reused by the next one)
            ACX_HIP(c, hipStreamSynchronize(c->stream));
        }
        return ACX_OK;
    });
}

// ---- debug: what a kernel finds in memory it did not write ("Device blocks of a context") --------------
int acx_debug_set_alloc_fill(int on, uint32_t word)
{
    acx::g_alloc_fill.on = on != 0;
    acx::g_alloc_fill.word = word;
    return ACX_OK;
}

int acx_debug_fill_arenas(acx_ctx *c, uint32_t word)
{
    if (!c) return ACX_ERR_INVALID;
    ACX_HIP(c, hipSetDevice(c->device));
    return guarded(c, [&]() -> int {
        ACX_HIP(c, hipStreamSynchronize(c->stream));
        if (c->qstream) ACX_HIP(c, hipStreamSynchronize(c->qstream));
        if (c->qstream2) ACX_HIP(c, hipStreamSynchronize(c->qstream2));
        // every SCRATCH block of DESIGN.md's table, to capacity (pools and descriptors keep their contents; d_pbox, a descriptor, is
        // filled with the path pass's other blocks: its boxes are uploaded before every launch)
        for (Serra09Slot &S : c->slot) {
            ACX_HIP(c, S.d_out.fill(word));
            ACX_HIP(c, S.d_al.fill(word));
            ACX_HIP(c, S.d_nsec.fill(word));
        }
        for (DeviceBuffer<float> *b : {&c->d_scratch, &c->d_thr, &c->d_out, &c->rank_d[0], &c->rank_d[1]}) ACX_HIP(c, b->fill(word));
        for (DeviceBuffer<double> *b : {&c->d_out64, &c->d_spmp}) ACX_HIP(c, b->fill(word));
        for (DeviceBuffer<unsigned> *b : {&c->d_efbits, &c->d_efdir, &c->d_efctr}) ACX_HIP(c, b->fill(word));
        for (DeviceBuffer<unsigned long long> *b : {&c->d_bits, &c->d_dir}) ACX_HIP(c, b->fill(word));
        for (DeviceBuffer<int32_t> *b : {&c->d_spmpi, &c->d_pcells, &c->d_pn, &c->d_efres}) ACX_HIP(c, b->fill(word));
        ACX_HIP(c, c->d_sprec.fill(word));
        ACX_HIP(c, c->d_seam.fill(word));
        ACX_HIP(c, c->d_pseam.fill(word));
        ACX_HIP(c, c->d_pbox.fill(word));
        ACX_HIP(c, c->d_nf.fill(word));
        ACX_HIP(c, hipDeviceSynchronize());
        return ACX_OK;
    });
}

// ---- device buffers for hosts that hold no GPU runtime of their own ------------------------------------------
int acx_dev_alloc(acx_ctx *c, int64_t bytes, void **d_ptr)
{
    if (!c) return ACX_ERR_INVALID;
    if (bytes < 0 || !d_ptr) return fail(c, ACX_ERR_INVALID, "dev_alloc: bad argument");
    ACX_HIP(c, hipSetDevice(c->device));
    DeviceBuffer<char> buf;
    const hipError_t e = buf.grow((size_t)std::max<int64_t>(bytes, 4));
    if (e != hipSuccess) return fail(c, ACX_ERR_NOMEM, std::string("dev_alloc: ") + hipGetErrorString(e));
    ACX_HIP(c, hipMemsetAsync(buf, 0, buf.capacity(), c->stream));
    ACX_HIP(c, hipStreamSynchronize(c->stream));
    *d_ptr = buf.get();
    c->dev_bufs.push_back(std::move(buf));
    return ACX_OK;
}

int acx_dev_free(acx_ctx *c, void *d_ptr)
{
    if (!c) return ACX_ERR_INVALID;
    auto it = std::find_if(c->dev_bufs.begin(), c->dev_bufs.end(), [&](const DeviceBuffer<char> &b) { return b.get() == d_ptr; });
    if (it == c->dev_bufs.end()) return fail(c, ACX_ERR_INVALID, "dev_free: not a buffer of this context");
    ACX_HIP(c, hipSetDevice(c->device));
    ACX_HIP(c, hipStreamSynchronize(c->stream));
    const hipError_t e = it->reset();
    c->dev_bufs.erase(it);
    ACX_HIP(c, e);
    return ACX_OK;
}

int acx_dev_read(acx_ctx *c, void *host_dst, const void *d_src, int64_t bytes)
{
    if (!c) return ACX_ERR_INVALID;
    if (!host_dst || !d_src || bytes < 0) return fail(c, ACX_ERR_INVALID, "dev_read: bad argument");
    ACX_HIP(c, hipSetDevice(c->device));
    ACX_HIP(c, hipStreamSynchronize(c->stream));
    if (bytes > 0) ACX_HIP(c, hipMemcpy(host_dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost));
    return ACX_OK;
}

int acx_dev_sync(acx_ctx *c)
{
    if (!c) return ACX_ERR_INVALID;
    ACX_HIP(c, hipSetDevice(c->device));
    ACX_HIP(c, hipDeviceSynchronize());
    return ACX_OK;
}

// ---- RCCL inside the library: a C host gets the multi-GPU pair grid without torch ---------------------------
// librccl is found at run time (no link dependency: single-GPU users never load it): ACX_RCCL_LIB, a copy the
// process already holds (PyTorch-ROCm bundles one), the one next to the HIP runtime in use, the system's.
namespace {
struct RcclApi {
    void *handle = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    std::string path, error;
};
RcclApi g_rccl;

bool rccl_load()
{
    if (g_rccl.handle) return true;
    std::vector<std::string> cand;
    void *h = nullptr;
    const char *forced = getenv("ACX_RCCL_LIB");          // an explicit choice is the ONLY candidate: a wrong path fails loudly
    if (forced && forced[0]) {
        cand.push_back(forced);
    } else {
        for (const char *n : {"librccl.so", "librccl.so.1"})                 // a copy this process already holds
            if (!h && (h = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) g_rccl.path = std::string(n) + " (already loaded)";
        if (!h) {
            Dl_info info;
            if (dladdr((void *)hipGetDeviceCount, &info) && info.dli_fname) {       // next to the HIP runtime in use
                std::string d(info.dli_fname);
                const size_t k = d.rfind('/');
                if (k != std::string::npos) { cand.push_back(d.substr(0, k) + "/librccl.so"); cand.push_back(d.substr(0, k) + "/librccl.so.1"); }
            }
            cand.push_back("librccl.so.1");
            cand.push_back("librccl.so");
            cand.push_back("/opt/rocm/lib/librccl.so");
        }
    }
    std::string why;
    for (const std::string &p : cand) {
        if (h) break;
        if ((h = dlopen(p.c_str(), RTLD_NOW | RTLD_GLOBAL))) { g_rccl.path = p; break; }
        const char *e = dlerror();                          // (one call: dlerror() clears the message it returns)
        if (e) why = e;
    }
    if (!h) { g_rccl.error = std::string("librccl.so not found (set ACX_RCCL_LIB): ") + why; return false; }
#define ACX_SYM(F_) g_rccl.F_ = reinterpret_cast<decltype(g_rccl.F_)>(dlsym(h, "nccl" #F_)); \
    if (!g_rccl.F_) { g_rccl.error = "librccl (" + g_rccl.path + ") lacks nccl" #F_; dlclose(h); return false; }
    ACX_SYM(GetUniqueId) ACX_SYM(CommInitRank) ACX_SYM(AllGather) ACX_SYM(CommDestroy) ACX_SYM(GetErrorString)
#undef ACX_SYM
    g_rccl.handle = h;
    return true;
}
}  // namespace

static void comm_release(acx_ctx *c)
{
    if (c->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c->comm);
    c->comm = nullptr;
    c->comm_world = 0;
    c->comm_rank = 0;
}

int acx_comm_id(void *id_out)
{
    if (!id_out) return ACX_ERR_INVALID;
    static_assert(sizeof(ncclUniqueId) == ACX_COMM_ID_BYTES, "ACX_COMM_ID_BYTES is sizeof(ncclUniqueId)");
    if (!rccl_load()) { g_create_error = g_rccl.error; return ACX_ERR_UNSUPPORTED; }
    ncclUniqueId id;
    const ncclResult_t r = g_rccl.GetUniqueId(&id);
    if (r != ncclSuccess) { g_create_error = std::string("ncclGetUniqueId: ") + g_rccl.GetErrorString(r); return ACX_ERR_HIP; }
    memcpy(id_out, &id, sizeof(id));
    return ACX_OK;
}

int acx_comm_init(acx_ctx *c, const void *id, int32_t rank, int32_t world)
{
    if (!c) return ACX_ERR_INVALID;
    if (!id || world < 1 || rank < 0 || rank >= world) return fail(c, ACX_ERR_INVALID, "comm_init: bad argument");
    if (c->comm) return fail(c, ACX_ERR_STATE, "comm_init: this context already holds a communicator (acx_comm_destroy first)");
    if (!rccl_load()) return fail(c, ACX_ERR_UNSUPPORTED, "comm_init: " + g_rccl.error);
    ACX_HIP(c, hipSetDevice(c->device));
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof(uid));
    ncclComm_t comm = nullptr;
    const ncclResult_t r = g_rccl.CommInitRank(&comm, world, uid, rank);
    if (r != ncclSuccess) return fail(c, ACX_ERR_HIP, std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(r));
    c->comm = comm;
    c->comm_rank = rank;
    c->comm_world = world;
    return ACX_OK;
}

int acx_comm_destroy(acx_ctx *c)
{
    if (!c) return ACX_ERR_INVALID;
    ACX_HIP(c, hipSetDevice(c->device));
    ACX_HIP(c, hipStreamSynchronize(c->stream));
    comm_release(c);
    return ACX_OK;
}

int acx_grid_allgather(acx_ctx *c, const float *d_local, float *d_gathered, int64_t floats_per_rank)
{
    if (!c) return ACX_ERR_INVALID;
    if (!c->comm) return fail(c, ACX_ERR_STATE, "grid_allgather: no communicator (acx_comm_init)");
    if (!d_local || !d_gathered || floats_per_rank < 1) return fail(c, ACX_ERR_INVALID, "grid_allgather: bad argument");
    ACX_HIP(c, hipSetDevice(c->device));
    // on the library's own stream: ordered behind the kernels of acx_grid_run, no host fence in between
    const ncclResult_t r = g_rccl.AllGather(d_local, d_gathered, (size_t)floats_per_rank, ncclFloat32, c->comm, c->stream);
    if (r != ncclSuccess) return fail(c, ACX_ERR_HIP, std::string("ncclAllGather: ") + g_rccl.GetErrorString(r));
    ACX_HIP(c, hipStreamSynchronize(c->stream));
    return ACX_OK;
}

// The whole N x N grid over the ranks of the communicator: plan (identical on every rank), this rank's tiles
// into its device buffer, ONE all-gather of the rank buffers over RCCL, rank 0 copies the gathered buffers to
// the host and scatters them into the caller's planes -- acoss_amd/algorithms/algorithm_template.py
// `_all_pairwise_grid` for a host without Python (reference: algorithm_template.py:168-192).
int acx_pair_grid_ranks(acx_ctx *c, const acx_grid_spec *spec_in, const void *params, float *const *D, int64_t ld, int32_t mirror)
{
    // A COLLECTIVE: what can differ between the ranks (rank 0's planes, a rank's pool, its device memory, its kernels) must
    // not make one rank return while the others wait in the all-gather.  Only checks that come out the same on every rank
    // return early; everything else becomes this rank's STATUS, which travels with the exchanges: one float per rank ahead
    // of the tiles (a rank that cannot even allocate its buffers is seen by all before anybody starts) and one appended to
    // every rank's score buffer (a rank whose kernels failed).  Any non-zero status fails the call on EVERY rank and rank 0
    // scatters nothing.
    if (!c) return ACX_ERR_INVALID;
    if (!c->comm) return fail(c, ACX_ERR_STATE, "pair_grid_ranks: no communicator (acx_comm_init)");
    if (!spec_in || (!params && spec_in->algo != ACX_ALGO_FTM2D)) return fail(c, ACX_ERR_INVALID, "pair_grid_ranks: bad argument");
    acx_grid_spec spec = *spec_in;
    spec.world = c->comm_world;
    if (!acx::grid_spec_ok(&spec)) return fail(c, ACX_ERR_INVALID, "pair_grid_ranks: bad grid spec");
    const int w = acx::grid_planes(spec.algo);
    const int world = spec.world;
    ACX_HIP(c, hipSetDevice(c->device));
    DeviceBuffer<float> d_st;                                   // [0] this rank's status, [1 .. world] everybody's
    ACX_HIP(c, d_st.grow((size_t)world + 1));
    int st = ACX_OK;
    std::string why;
    auto local_fail = [&](int code, const std::string &msg) { if (st == ACX_OK) { st = code; why = msg; } };
    if (c->comm_rank == 0) {
        if (!D) local_fail(ACX_ERR_INVALID, "pair_grid_ranks: rank 0 needs the planes");
        else for (int e = 0; e < w; ++e) if (!D[e]) local_fail(ACX_ERR_INVALID, "pair_grid_ranks: null plane");
    }
    std::vector<int64_t> len;
    {
        const int rl = pool_lengths(c, spec.algo, len);
        if (rl != ACX_OK) local_fail(rl, acx_last_error(c));
    }
    if (st == ACX_OK && c->comm_rank == 0 && ld < (int64_t)len.size())
        local_fail(ACX_ERR_INVALID, "pair_grid_ranks: leading dimension smaller than the number of tracks");
    std::vector<acx_grid_tile> tiles;
    std::vector<int64_t> fl;
    std::vector<double> co;
    int64_t stride = 1;
    DeviceBuffer<float> d_local, d_all;
    if (st == ACX_OK) {
        acx::grid_plan(len.data(), (int)len.size(), spec, tiles, fl, co);
        for (int r = 0; r < world; ++r) stride = std::max(stride, fl[r]);
        // (+ 1: the status float behind the tiles)
        if (d_local.grow((size_t)(stride + 1)) != hipSuccess || d_all.grow((size_t)(stride + 1) * world) != hipSuccess) {
            local_fail(ACX_ERR_NOMEM, "pair_grid_ranks: the gathered score buffers do not fit the device");
        }
    }
    // every rank's status, before any rank starts its tiles
    std::vector<float> hst((size_t)world + 1, 0.0f);
    auto exchange_status = [&](int mine) -> int {                // returns the first failing rank, -1 if none, -2 on a HIP / RCCL error
        const float f = (float)mine;
        if (hipMemcpy(d_st, &f, sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return -2;      // (nothing is pending on the stream)
        if (acx_grid_allgather(c, d_st, d_st + 1, 1) != ACX_OK) return -2;
        if (hipMemcpy(hst.data(), d_st + 1, sizeof(float) * (size_t)world, hipMemcpyDeviceToHost) != hipSuccess) return -2;
        for (int r = 0; r < world; ++r) if (hst[r] != 0.0f) return r;
        return -1;
    };
    auto fail_all = [&](int bad_rank) -> int {
        if (bad_rank == -2) return fail(c, ACX_ERR_HIP, "pair_grid_ranks: the status exchange failed");
        if (st != ACX_OK) return fail(c, st, why);
        return fail(c, (int)hst[bad_rank], "pair_grid_ranks: rank " + std::to_string(bad_rank) + " failed (its own context holds the message)");
    };
    int bad = exchange_status(st);
    if (bad != -1) return fail_all(bad);
    (void)hipMemsetAsync(d_local, 0, sizeof(float) * (size_t)(stride + 1), c->stream);
    const int rc = acx_grid_run(c, &spec, params, c->comm_rank, 0, -1, d_local);
    if (rc != ACX_OK) { st = rc; why = acx_last_error(c); }
    {
        const float f = (float)st;
        // (acx_grid_run returns with its stream drained, the memset included: a plain copy cannot race it)
        if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(d_local + stride, &f, sizeof(float), hipMemcpyHostToDevice) != hipSuccess) (void)hipGetLastError();
    }
    // (a rank whose tiles failed still joins: the others must not be left waiting, and they learn about it from the status float)
    const int rg = acx_grid_allgather(c, d_local, d_all, stride + 1);
    if (rg != ACX_OK) return rg;
    if (hipMemcpy2D(hst.data(), sizeof(float), d_all + stride, sizeof(float) * (size_t)(stride + 1), sizeof(float), (size_t)world,
                    hipMemcpyDeviceToHost) != hipSuccess) return fail_all(-2);
    bad = -1;
    for (int r = 0; r < world; ++r) if (hst[r] != 0.0f) { bad = r; break; }
    if (bad != -1) return fail_all(bad);
    int out = ACX_OK;
    if (c->comm_rank == 0) {
        std::vector<float> h((size_t)(stride + 1) * world);
        const hipError_t e = hipMemcpy(h.data(), d_all, sizeof(float) * h.size(), hipMemcpyDeviceToHost);
        if (e != hipSuccess) out = fail(c, ACX_ERR_HIP, std::string("pair_grid_ranks: ") + hipGetErrorString(e));
        else acx::grid_scatter(tiles, spec, h.data(), stride + 1, 0, -1, D, ld, mirror);
    }
    return out;
}

// The device a context would run on, for hosts that have to PROVE which GPU each of their ranks holds (bench.py's `ranks`
// array): PCI bus id ("0000:c1:00.0"), marketing name, gcn arch, and how many devices this process can see.
int acx_device_info(int device, char *pci_bus_id, int pci_len, char *name, int name_len, int *visible)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return ACX_ERR_HIP;
    if (visible) *visible = n;
    if (device < 0 || device >= n) return ACX_ERR_INVALID;
    if (pci_bus_id && pci_len > 0 && hipDeviceGetPCIBusId(pci_bus_id, pci_len, device) != hipSuccess) return ACX_ERR_HIP;
    if (name && name_len > 0) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) != hipSuccess) return ACX_ERR_HIP;
        snprintf(name, (size_t)name_len, "%s (%s)", prop.name, prop.gcnArchName);
    }
    return ACX_OK;
}

int acx_profile_enable(acx_ctx *c, int on)
{
    if (!c) return ACX_ERR_INVALID;
    c->prof = on != 0;
    return ACX_OK;
}
int acx_profile_reset(acx_ctx *c)
{
    if (!c) return ACX_ERR_INVALID;
    for (auto &s : c->stats) { s.ms = 0; s.launches = 0; s.cells = 0; }
    return ACX_OK;
}
int acx_profile_count(const acx_ctx *c) { return c ? KS_COUNT : 0; }
int acx_profile_get(acx_ctx *c, int idx, char *name, int name_len, double *ms, int64_t *launches, int64_t *cells)
{
    if (!c || idx < 0 || idx >= KS_COUNT) return ACX_ERR_INVALID;
    if (name && name_len > 0) { strncpy(name, c->stats[idx].name, name_len - 1); name[name_len - 1] = 0; }
    if (ms) *ms = c->stats[idx].ms;
    if (launches) *launches = c->stats[idx].launches;
    if (cells) *cells = c->stats[idx].cells;
    return ACX_OK;
}


static int debug_sqrt(acx_ctx *c, const float *in, int64_t n, float *out, bool ef);
int acx_debug_sqrt(acx_ctx *c, const float *in, int64_t n, float *out) { return debug_sqrt(c, in, n, out, false); }
int acx_debug_ef_sqrt(acx_ctx *c, const float *in, int64_t n, float *out) { return debug_sqrt(c, in, n, out, true); }
static int debug_sqrt(acx_ctx *c, const float *in, int64_t n, float *out, bool ef)
{
    if (!c || !in || !out || n <= 0) return ACX_ERR_INVALID;
    ACX_HIP(c, hipSetDevice(c->device));
    DeviceBuffer<float> d_in, d_o;
    ACX_HIP(c, d_in.grow((size_t)n));
    ACX_HIP(c, d_o.grow((size_t)n));
    ACX_HIP(c, hipMemcpy(d_in, in, sizeof(float) * n, hipMemcpyHostToDevice));
    if (ef) hipLaunchKernelGGL(acx::ef_sqrt_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, d_in.get(), d_o.get(), n);
    else hipLaunchKernelGGL(acx::sqrt_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, d_in.get(), d_o.get(), n);
    ACX_HIP(c, hipStreamSynchronize(c->stream));
    ACX_HIP(c, hipMemcpy(out, d_o, sizeof(float) * n, hipMemcpyDeviceToHost));
    return ACX_OK;
}

}  // extern "C"
