/*
 * acx.h -- C ABI of libacx.so, the MI355X (gfx950) all-pairwise cover-song
 * similarity engine behind acoss's CoverAlgorithm.similarity()/all_pairwise().
 *
 * The reference (furkanyesiler/acoss) is pure Python and has NO FFI of its own;
 * its only native boundary on this path is essentia's Python wrapper
 * (acoss/algorithms/rqa_serra09.py:60-67).  Each entry point below therefore
 * cites the reference INTERFACE it replaces; INTEGRATION.md shows the ctypes
 * binding a maintainer adds on the acoss side.
 *
 * Conventions
 *   - plain C types only; every host buffer is caller-allocated and
 *     caller-owned; the library owns device memory inside acx_ctx; no pointer
 *     outlives a call except the context.
 *   - every call returns ACX_OK (0) or a negative ACX_ERR_* code; the message
 *     is available from acx_last_error().  Nothing falls back to the CPU.
 *   - a context is single-owner (one host thread per context / per GPU).
 */
#ifndef ACX_H
#define ACX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 4): + acx_dev_alloc / _free / _read / _sync, acx_comm_id / _init / _destroy, acx_grid_allgather,
 *              acx_pair_grid_ranks; acx_ef_pool_end fails on tracks never handed over; uploads reject non-finite input
 *              (since the round-3 library, which still said 1).  The ctypes shim refuses a library of another version. */
/* 3 (round 5): + acx_device_info; acx_pair_grid_ranks carries a per-rank status through its exchanges (a failing rank fails the call
 *              on every rank instead of leaving the others in the all-gather); ACX_RCCL_LIB, when set, is the only librccl tried. */
#define ACX_ABI_VERSION 4

enum {
    ACX_OK = 0,
    ACX_ERR_INVALID = -1,      /* bad argument (NULL, index out of range, dim != expected)  */
    ACX_ERR_HIP = -2,          /* a HIP runtime call failed / no gfx950 device              */
    ACX_ERR_NOMEM = -3,        /* device scratch cannot hold even one pair                  */
    ACX_ERR_STATE = -4,        /* pool not uploaded                                         */
    ACX_ERR_SHORT = -5,        /* a track is shorter than the delay-embedding stack (essentia
                                  raises EssentiaException there)                           */
    ACX_ERR_UNSUPPORTED = -6   /* parameter combination not implemented on the device       */
};

typedef struct acx_ctx acx_ctx;

/* ---- context ------------------------------------------------------------ */

/* Create a context on HIP device `device`.  Returns NULL and sets *err on failure. */
acx_ctx *acx_create(int device, int *err);
void acx_destroy(acx_ctx *ctx);
/* Last error message of this context (ctx == NULL: of the last failed acx_create). */
const char *acx_last_error(const acx_ctx *ctx);
int acx_abi_version(void);
/* HIP_VERSION the library was compiled against and the version of the HIP runtime it is running on (0: unknown).
 * The ctypes shim records both (acoss_amd._lib.HIP_VERSIONS) and warns when the MAJOR versions differ; a process
 * that also holds PyTorch-ROCm runs on the runtime torch bundles (this image: built against 7.2, runs on 7.0 --
 * same major, recorded, no warning). */
int acx_hip_versions(int *build, int *runtime);
/* Which GPU is HIP device `device` of this process: PCI bus id ("0000:c1:00.0"), "name (gcn arch)", and the number of
 * devices the process can see (HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES applied).  bench.py gathers one of these per
 * rank and refuses to report a multi-GPU figure when two ranks hold the same device.  No reference counterpart
 * (joblib workers share one host, algorithm_template.py:172-177). */
int acx_device_info(int device, char *pci_bus_id, int pci_len, char *name, int name_len, int *visible);
/* Upper bound (bytes) for the per-batch device scratch; 0 restores the default: env ACX_SCRATCH_GB, else 40 % of
 * device memory for the Serra09 batches and min(40 %, 36 GB) for the EarlyFusion arena (what one 128 x 128 grid tile
 * of 300-500-block tracks needs; larger arenas only cost allocation time). */
int acx_set_scratch_limit(acx_ctx *ctx, int64_t bytes);

/* ---- feature pool ------------------------------------------------------- */

/*
 * What an upload does with non-finite feature values.  Real feature files carry them -- the reference
 * zeroes NaN MFCCs itself (earlyfusion_traile.py:105) and hands everything else to essentia / numpy
 * unchecked, where one NaN frame spoils the scores of its own track.  Here it would spoil more: the
 * band kernel reads a neighbouring track's frames for the cells beyond a matrix's edge.  So every
 * acx_*upload* call scans what it receives, on the device:
 *   ACX_NONFINITE_REJECT (default)  the upload fails with ACX_ERR_INVALID, the message names the first
 *                                   offending track; no pool is left behind
 *   ACX_NONFINITE_ZERO              NaN / Inf values are replaced by 0 (what the reference does for MFCCs);
 *                                   acx_nonfinite_zeroed() tells how many the last upload replaced
 * NaN MFCC samples (acx_ef_block_features / acx_ef_upload_raw_pool) are zeroed under either policy.
 */
enum { ACX_NONFINITE_REJECT = 0, ACX_NONFINITE_ZERO = 1 };
int acx_set_nonfinite_policy(acx_ctx *ctx, int32_t policy);
int64_t acx_nonfinite_zeroed(const acx_ctx *ctx);

/*
 * Upload the packed feature pool: `frames` is row-major (sum_i T_i, dim) f32,
 * track i occupies rows offsets[i] .. offsets[i+1].  Replaces the per-track
 * feature cache of the reference (Serra09.load_features -> self.all_feats,
 * rqa_serra09.py:44-53): tracks are ALREADY pooled (x40 median) when uploaded.
 * dim must be 12 for the chroma algorithms.  Copies to HBM; the host buffers may
 * be released on return.
 */
int acx_upload_pool(acx_ctx *ctx, const float *frames, const int64_t *offsets,
                    int32_t n_tracks, int32_t dim);

/*
 * The same pool from RAW chroma: `raw` is row-major (sum_i T0_i, 12) f32, track i occupies rows
 * raw_offsets[i] .. raw_offsets[i+1]; the device takes the median over consecutive blocks of
 * `fac` frames (the last block of a track may be shorter) -- what Serra09.load_features does per
 * track with librosa.util.sync(chroma.T, arange(0, T0, fac), aggregate=np.median).T
 * (rqa_serra09.py:49-52; downsample_fac = 40 by default, <= 64 here).  Bit-identical to np.median
 * on f32 input.  pooled_offsets_out (n_tracks + 1 entries, may be NULL) receives the offsets of
 * the pooled tracks: ceil(T0_i / fac) frames each.
 */
int acx_upload_raw_pool(acx_ctx *ctx, const float *raw, const int64_t *raw_offsets, int32_t n_tracks,
                        int32_t dim, int32_t fac, int64_t *pooled_offsets_out);

/* Copy the f32 pool back (tests): `frames` has room for `capacity` floats. */
int acx_download_pool(acx_ctx *ctx, float *frames, int64_t capacity);

/* ---- Serra09 (OTI + delay embedding + CSM + mutual-kappa + Qmax) --------- */

/* Mirrors the constructor arguments of Serra09 (rqa_serra09.py:31-32) that reach
 * essentia (rqa_serra09.py:60-64), plus the switchable recalled-essentia details
 * documented in oracle/acx_oracle.c. */
typedef struct {
    int32_t m;           /* frameStackSize,   default 9 (device: 1..33) */
    int32_t tau;         /* frameStackStride, default 1 */
    float kappa;         /* binarizePercentile, default 0.095 */
    int32_t oti;         /* default 1 */
    float gamma_o;       /* disOnset, default 0.5 */
    float gamma_e;       /* disExtension, default 0.5 */
    int32_t embed_full;  /* 0: M = T - m*tau   1: M = T - (m-1)*tau */
    int32_t pct_mode;    /* 0 linear  1 essentia d0+d1  2 lower  3 nearest.  Position k = (n - 1) kappa; 0 and 1 both
                            interpolate d_(floor k) (ceil k - k) + d_(ceil k) (k - floor k) and differ only when k is an
                            exact integer: 1 evaluates the formula as recalled from essentia -- both weights are 0, the
                            threshold is 0 and the row stays empty (rows of n - 1 = 200, 400, ... cells at kappa =
                            0.095) --, 0 (the default, a DELIBERATE deviation until the pin kit says otherwise)
                            returns d_(k), the value the interpolation converges to.
                            tests/test_oracle_serra09.py::test_integer_percentile_position pins both. */
    int32_t oti_target;  /* 0 rotate reference  1 rotate query */
    int32_t dp_start;    /* 2 or 3 */
    int32_t inclusive;   /* 1: d <= eps  0: d < eps */
    int32_t dmax;        /* 0 Qmax ('serra09')  1 Dmax ('chen17') */
    int32_t arith;       /* ACX_ARITH_EXACT (default) or ACX_ARITH_F16X2, see below (ABI 2: new last field) */
} acx_serra09_params;

/*
 * Arithmetic of the frame Gram behind the distance matrix (everything else is the same code in both):
 *   ACX_ARITH_EXACT  v_mfma_f32_16x16x4_f32 chains: the f32 spec the oracle reproduces bit for bit
 *   ACX_ARITH_F16X2  opt-in, m = 9 only: every bin value as two fp16 terms x = h1 + h2 (22-23 significant bits; the matrix pipe
 *                    keeps fp16 subnormals), products x1 y1 + x1 y2 + x2 y1 + x2 y2 on two v_mfma_f32_16x16x32_f16, which run
 *                    beside other waves' VALU work where an f32 MFMA blocks the SIMD.  As accurate as the f32 chain against f64
 *                    (2e-7 relative, scripts/ubench/mfma_f16_probe.hip) but NOT the same bits: scores are graded by north_star's
 *                    tolerance (|score difference| <= 2.0, identical MAP / MR on cover sets; tests/test_gpu_serra09.py), the
 *                    default and bench.py's headline stay exact.  Pairs beyond the band kernel (rows of more than 2041 cells)
 *                    take the exact streaming kernels in either mode.  INPUT RANGE: the first term must be finite, and the
 *                    second is rounded to fp16's subnormal step of 2^-24, an absolute error that doubles relative to the
 *                    features with every halving of them -- a pool whose largest magnitude lies outside [2^-1, 2^15] is
 *                    refused with ACX_ERR_UNSUPPORTED (HPCP / CREMA frames are normalised to a maximum of 1; rescale anything
 *                    else by a power of two).  Inside that range squared distances of frame-max-normalised features lie within
 *                    3e-5 x (largest magnitude)^2 of f64 (1.3e-5 measured; the exact chain: 1.2e-5), and the recurrence plot is
 *                    the f64 plot on every cell those distances decide (tests/test_gpu_serra09_f16x2.py).
 */
enum { ACX_ARITH_EXACT = 0, ACX_ARITH_F16X2 = 1 };

void acx_serra09_default_params(acx_serra09_params *p);

/*
 * Scores for K (query, reference) track-index pairs: out[k] = max of the Qmax
 * matrix for pair (pairs[2k], pairs[2k+1]) -- exactly the scalar that
 * Serra09.similarity() stores into Ds[key][i][j] (rqa_serra09.py:55-69), for a
 * whole (K,2) idxs array in one call instead of one essentia round trip per pair.
 * pairs, out: host memory.  The pool must be uploaded.
 */
int acx_serra09_pairs(acx_ctx *ctx, const int32_t *pairs, int64_t K,
                      const acx_serra09_params *params, float *out);

/*
 * ChenFusion (latefusion_chen.py:58-72): for every pair ONE cross recurrence plot and two
 * alignments of it -- out[2k] = Qmax ('serra09'), out[2k+1] = Dmax ('chen17') -- the two
 * scalars ChenFusion.similarity() stores into Ds["qmax"][i][j] and Ds["dmax"][i][j].
 * params->dmax is ignored.  out: 2*K floats, host memory.
 */
int acx_chenfusion_pairs(acx_ctx *ctx, const int32_t *pairs, int64_t K,
                         const acx_serra09_params *params, float *out);

/*
 * One pair with intermediates, for parity tests (every pointer may be NULL):
 *   d2   (Mq*Mr) squared embedded distances (the ChromaCrossSimilarity distance
 *        matrix before sqrt, rqa_serra09.py:66)
 *   epsq (Mq), epsr (Mr)   the kappa-percentile thresholds on d = sqrt(d2)
 *   thrq (Mq), thrr (Mr)   the same thresholds moved to the d2 domain
 *                          (largest f32 x with sqrt(x) <=/< eps)
 *   oti, score, dims[2] = {Mq, Mr}
 * To hand back d2 and the thresholds this entry runs the D2-WRITING instantiations of the band
 * kernels, with the thresholds' d-domain values kept, on one stream, one pair per batch: not the
 * kernels acx_serra09_pairs launches.  acx_serra09_debug_bits observes those.
 */
int acx_serra09_debug_pair(acx_ctx *ctx, int32_t i, int32_t j,
                           const acx_serra09_params *params,
                           float *d2, float *epsq, float *epsr,
                           float *thrq, float *thrr,
                           int32_t *oti, float *score, int32_t *dims);

/*
 * The recurrence plots of the PRODUCT path, for parity tests: runs exactly what acx_serra09_pairs
 * runs for the list (same kernels, same size-class sort, same streams; scores: K floats) and then
 * copies the batch's recurrence bitmaps back and unpacks them on the host:
 *   R_out   uint8 (Mq_k x Mr_k) plots, row-major, concatenated in the order of `pairs`
 *           (sum of Mq_k * Mr_k bytes)
 *   outside (may be NULL) number of set bits found in the pairs' bitmap words at columns outside
 *           [0, Mr).  The alignment sweeps do not rely on these being zero: every sweep kernel
 *           masks the columns left of 0 and right of the matrix itself, so this is a figure to
 *           report, not an invariant.
 * The list must fit ONE batch (the scratch limit, 65535 pairs); otherwise ACX_ERR_UNSUPPORTED and
 * nothing is launched.  Validation is acx_serra09_pairs'.
 */
int acx_serra09_debug_bits(acx_ctx *ctx, const int32_t *pairs, int64_t K,
                           const acx_serra09_params *params, float *scores,
                           uint8_t *R_out, int64_t *outside);

/*
 * The alignment alone (tests): Qmax ('serra09', params->dmax = 0) or Dmax ('chen17', dmax = 1) of a
 * given binary (M, N) uint8 cross recurrence plot -- the scalar CoverSongSimilarity returns for the
 * matrix ChromaCrossSimilarity produced (rqa_serra09.py:64,67; latefusion_chen.py:68-71).  Uses
 * params->gamma_o, gamma_e, dp_start, dmax; any M, N.  Non-{0,1} input -> ACX_ERR_INVALID.
 */
int acx_qmax_binary(acx_ctx *ctx, const uint8_t *R, int32_t M, int32_t N, const acx_serra09_params *params,
                    float *score);

/*
 * WHERE the Qmax alignment lies.  Q is the matrix whose maximum acx_serra09_pairs returns.
 *   score      max Q: the bits acx_serra09_pairs returns for the pair
 *   (q1, r1)   end: the first cell in row-major order (smallest row, then smallest column) at which Q attains it
 *   (q0, r0)   start: follow predecessors from the end until a cell has none.  Predecessor of a match cell: the first of
 *              Q[i-1][j-1], Q[i-2][j-1], Q[i-1][j-2] equal to their maximum, none when that maximum is 0; of a gap cell
 *              with Q > 0: the first of the three penalised values equal to their maximum.
 * Coordinates are rows (query) and columns (reference) of the recurrence plot, i.e. EMBEDDED frames (with dp_start == 3 the
 * oracle's DP cell (i, j) reads R[i-1][j-1]: reported is the R index).  score == 0: no match, all four are -1.
 * Qmax only: params->dmax != 0 -> ACX_ERR_UNSUPPORTED before any launch.
 */
typedef struct { float score; int32_t q0, r0, q1, r1; } acx_alignment;

/*
 * The alignments of K (query, reference) pairs over the uploaded pool: the chain of acx_serra09_pairs (the same validation
 * of the whole list before the first launch, batch plan, class sort and band / streaming kernels under params->arith), with
 * qmax_locate_kernel as the sweep of every class, one wave per pair.  out: K records in the order of `pairs`.
 */
int acx_serra09_align(acx_ctx *ctx, const int32_t *pairs, int64_t K, const acx_serra09_params *params, acx_alignment *out);

/*
 * The same DP alone on a given binary (M, N) uint8 plot, like acx_qmax_binary: uses params->gamma_o, gamma_e, dp_start;
 * any M, N.  Non-{0,1} input -> ACX_ERR_INVALID; params->dmax != 0 -> ACX_ERR_UNSUPPORTED.
 */
int acx_qmax_locate_binary(acx_ctx *ctx, const uint8_t *R, int32_t M, int32_t N, const acx_serra09_params *params,
                           acx_alignment *out);

/*
 * The PATH of the Qmax alignment: the cells from the start (q0, r0) to the end (q1, r1), both included, that
 * the predecessor chain from the end visits -- rows and columns of the recurrence plot, the coordinates of acx_alignment, listed from
 * start to end; consecutive cells differ by (1, 1), (2, 1) or (1, 2); a pair without a match has an empty path.  A second pass behind
 * the locating sweep of every batch (qmax_path_kernel): the Qmax recursion over the cells of the reported box only, one 2-bit
 * predecessor code per cell, and a traceback over the codes.
 *   out       K records, bit for bit what acx_serra09_align returns for the same arguments
 *   path_off  K + 1 entries: pair k's cells are cells[2 * path_off[k] .. 2 * path_off[k + 1]), (q, r) interleaved
 *   cells     cap x 2 int32
 *   cap       checked before the first launch against the bound the host knows then, the sum over the list of min(Mq_k, Mr_k) in
 *             embedded frames (no path has more cells than its plot's shorter side): too small -> ACX_ERR_INVALID with the required
 *             number in the message, nothing launched
 * The boxes of a batch run in chunks whose direction planes (2 bits per box cell) and seam records fit HALF the scratch limit
 * (acx_set_scratch_limit); a single box beyond that: ACX_ERR_NOMEM, nothing left in flight.  All other errors are those of
 * acx_serra09_align with the same codes; params->dmax != 0 -> ACX_ERR_UNSUPPORTED before anything else.
 */
int acx_serra09_align_paths(acx_ctx *ctx, const int32_t *pairs, int64_t K, const acx_serra09_params *params,
                            acx_alignment *out, int64_t *path_off /* K + 1 */, int32_t *cells /* cap x 2: (q, r) */, int64_t cap);

/*
 * The same DP alone on a given binary (M, N) uint8 plot, as acx_qmax_locate_binary is for the endpoints: `out` is its record,
 * *n_cells the number of cells written to `cells` (cap x 2 int32; cap >= min(M, N), else ACX_ERR_INVALID and nothing launched).
 */
int acx_qmax_path_binary(acx_ctx *ctx, const uint8_t *R, int32_t M, int32_t N, const acx_serra09_params *params,
                         acx_alignment *out, int64_t *n_cells, int32_t *cells, int64_t cap);

/*
 * EVERY matched section of a pair, not only the best one: an excerpt played twice, two halves with a solo
 * between them, a medley that quotes two passages of one reference.
 *   section 0      the alignment above: bit for bit acx_serra09_align's record, provided its score is >= min_score; else the pair has none
 *   free rows      the rows of the plot start as one free interval [0, Mq - 1].  A section with start row q0 and end row q1 that lies
 *                  in the free interval [a, b] EXCLUDES rows [max(a, q0 - pad), min(b, q1 + pad)] (the pad never reaches across an
 *                  earlier section); [a, b] is replaced by what is left above and below
 *   section k + 1  the alignment above of Q', the same recursion with Q' = 0 on every cell of an excluded row (NOT the recursion on a
 *                  plot with those rows cleared: a gap cell there would keep predecessor - gamma and bridge the stretch); reported iff
 *                  its score >= max(min_score, min_ratio * score_0) (one f32 multiply; equality counts)
 * The search ends at the first section that fails, or after max_sections.  Scores do not increase with k, the row ranges [q0, q1] of
 * a pair's sections are pairwise disjoint -- every QUERY frame belongs to at most one section --, reference columns may be shared
 * (the query repeats what the reference plays once; for a segmentation of the reference swap the pair).
 *   1 <= max_sections <= 16, pad >= 0, min_score > 1 (a score above 1 has two path cells: q1 > q0), 0 <= min_ratio <= 1;
 *   anything else -> ACX_ERR_INVALID before any launch.
 */
typedef struct { int32_t max_sections, pad; float min_score, min_ratio; } acx_section_opts;

/*
 * The sections of K (query, reference) pairs over the uploaded pool: the chain of acx_serra09_align (validation of the whole list
 * before the first launch, batch plan, class sort, band / streaming kernels, error codes and messages), then ONE launch of
 * qmax_sections_kernel per batch: one wave per pair, a sweep per free interval, the loop over sections inside the launch.
 *   out         K x max_sections records: pair k's sections at out[k * max_sections ..], section 0 first; beyond n_sections[k] the
 *               no-match record (score 0, -1 four times)
 *   n_sections  K counts
 *   path_off, cells, cap   both pointers NULL (cap ignored), or both given: the path of section s of pair k is
 *               cells[2 * path_off[k * max_sections + s] .. 2 * path_off[k * max_sections + s + 1]), as acx_serra09_align_paths lists
 *               a path (K * max_sections + 1 offsets); the path pass of section 17 over the sections' boxes, same budget and chunks.
 *               cap is checked before the first launch against the sum over the list of min(Mq_k, max_sections * min(Mq_k, Mr_k))
 *               (sections are row-disjoint, a path has at most as many cells as its box has rows): too small -> ACX_ERR_INVALID
 *               with the required number in the message
 * params->dmax != 0 -> ACX_ERR_UNSUPPORTED before anything else.
 */
int acx_serra09_align_sections(acx_ctx *ctx, const int32_t *pairs, int64_t K, const acx_serra09_params *params,
                               const acx_section_opts *opts, acx_alignment *out /* K x max_sections */, int32_t *n_sections /* K */,
                               int64_t *path_off /* K x max_sections + 1, or NULL */, int32_t *cells /* cap x 2, or NULL */, int64_t cap);

/*
 * The same DP alone on a given binary (M, N) uint8 plot, as acx_qmax_locate_binary / acx_qmax_path_binary are: out max_sections
 * records, *n_sections their number, path_off max_sections + 1 offsets; cap >= min(M, max_sections * min(M, N)).
 */
int acx_qmax_sections_binary(acx_ctx *ctx, const uint8_t *R, int32_t M, int32_t N, const acx_serra09_params *params,
                             const acx_section_opts *opts, acx_alignment *out, int32_t *n_sections,
                             int64_t *path_off, int32_t *cells, int64_t cap);

/*
 * LateFusionChen: where the alignment of ONE of the two planes of acx_chenfusion_pairs lies, and its path.
 * plane 0: Qmax -- byte for byte acx_serra09_align / acx_serra09_align_paths; plane 1: Dmax (dmax_locate_kernel, dmax_path_kernel);
 * any other value -> ACX_ERR_INVALID before any launch.  params->dmax is ignored, as in acx_chenfusion_pairs.
 * Dmax: Q is the oracle's matrix with dmax = 1 -- c3 = Q[i-2][j-1] + R[i-1][j], c4 = Q[i-1][j-2] + R[i][j-1] -- and
 *   score      max Q: the bits acx_chenfusion_pairs returns in column 1
 *   (q1, r1)   the row-major first cell that attains it
 *   (q0, r0)   follow predecessors from the end: the cell of the first candidate (bonus included; penalised in a gap cell) equal to the
 *              maximum of the three; a cell has none, and the path starts there, when Q of THAT cell (without its bonus) is 0.
 * The start cell's Q need not be 1, and the start can be a GAP cell whose bonus neighbour (q0 - 1, r0) or (q0, r0 - 1) is the recurrence
 * at which the alignment really begins: the span can begin one frame late.  Paths, steps, `cap`, chunks, budget and error codes are those
 * of acx_serra09_align_paths.
 */
int acx_chenfusion_align(acx_ctx *ctx, const int32_t *pairs, int64_t K, const acx_serra09_params *params, int32_t plane,
                         acx_alignment *out);
int acx_chenfusion_align_paths(acx_ctx *ctx, const int32_t *pairs, int64_t K, const acx_serra09_params *params, int32_t plane,
                               acx_alignment *out, int64_t *path_off /* K + 1 */, int32_t *cells /* cap x 2: (q, r) */, int64_t cap);

/*
 * The Dmax DP alone on a given binary (M, N) uint8 plot, as acx_qmax_locate_binary / acx_qmax_path_binary are for Qmax: uses
 * params->gamma_o, gamma_e, dp_start (params->dmax is ignored); any M, N.  Non-{0,1} input -> ACX_ERR_INVALID.
 */
int acx_dmax_locate_binary(acx_ctx *ctx, const uint8_t *R, int32_t M, int32_t N, const acx_serra09_params *params,
                           acx_alignment *out);
int acx_dmax_path_binary(acx_ctx *ctx, const uint8_t *R, int32_t M, int32_t N, const acx_serra09_params *params,
                         acx_alignment *out, int64_t *n_cells, int32_t *cells, int64_t cap);

/* Number of embedded frames for a pooled length T (0 if too short). */
int32_t acx_serra09_embed_len(int32_t T, const acx_serra09_params *params);

/*
 * The batch plan of a pair list, for tests and tools -- no context, no device: what acx_serra09_pairs /
 * acx_chenfusion_pairs would do with the list on a pool of these track lengths, told by the functions the run itself
 * calls (acoss_amd/csrc/serra09_plan.hpp; the per-process switches ACX_BAND2 / ACX_QMAX_MULTI / ACX_QMAX_STREAM apply).
 *   lengths       pooled frames per track, as uploaded (n_tracks of them); params->tau decimates them as the run does
 *   scratch_limit bytes, as acx_set_scratch_limit; 0: the default without a device -- env ACX_SCRATCH_GB, else unbounded
 *                 (a context's default is 40 % of ITS device's memory)
 *   out           K records, in the order of `pairs`:
 *     Mq, Mr                 embedded lengths (rows, columns of the pair's matrix)
 *     batch                  the batch the pair runs in (batches are contiguous runs of the list)
 *     cr, cq                 size classes 0..4 of its rows (Mr cells: row pass and sweep) and columns (Mq cells: column
 *                            pass); 5: the streaming kernels (then both are 5)
 *     row_family, col_family ACX_SERRA09_FAMILY_* of the band kernel of its row pass / column pass
 *     sweep_cols, sweep_pack the alignment sweep: bitmap columns a lane owns (0: the streaming sweep) and pairs per wave
 *                            (what the default penalties 0.5 / 0.5 run; other penalties take one wave per pair)
 * A list the run would refuse returns the run's code for it (ACX_ERR_INVALID: an index, ACX_ERR_SHORT: a track shorter
 * than the stack, ACX_ERR_NOMEM: a pair beyond the scratch limit, ACX_ERR_UNSUPPORTED: the parameters) and fills nothing.
 */
enum {
    ACX_SERRA09_FAMILY_BAND2_4ROWS = 0,   /* band2_kernel<M, B2_NV, 16>: four rows per wave, rows of <= 249 cells, m <= 9   */
    ACX_SERRA09_FAMILY_BAND2_2ROWS = 1,   /* band2_kernel<M, B2_NV, 32>: two rows per wave, <= 505 cells, m <= 9            */
    ACX_SERRA09_FAMILY_BAND2_MID = 2,     /* band2_kernel<M, B2_NV_MID, 32>: 24 positions per lane, <= 761 cells, m <= 9    */
    ACX_SERRA09_FAMILY_BAND_2 = 3,        /* band_kernel<M, 2>: 8 values per lane, <= 505 cells                             */
    ACX_SERRA09_FAMILY_BAND_4 = 4,        /* band_kernel<M, 4>: 16 values per lane, <= 1017 cells                           */
    ACX_SERRA09_FAMILY_BAND_8 = 5,        /* band_kernel<M, 8>: 32 values per lane, <= 2041 cells                           */
    ACX_SERRA09_FAMILY_STREAMING = 6      /* csm_long_kernel, rowsel_long_kernel, binarise_long_kernel: any length, m <= 33 */
};
typedef struct acx_serra09_plan_rec {
    int32_t Mq, Mr;
    int32_t batch;
    int32_t cr, cq;
    int32_t row_family, col_family;
    int32_t sweep_cols, sweep_pack;
} acx_serra09_plan_rec;
int acx_serra09_plan(const int64_t *lengths, int32_t n_tracks, const int32_t *pairs, int64_t K,
                     const acx_serra09_params *params, int64_t scratch_limit, acx_serra09_plan_rec *out);
/* Printable name of a family for stack size m (band_kernel's names tell m <= 9 from m >= 10: the same limits, another
 * kernel beside it); NULL for an unknown family.  The string is static. */
const char *acx_serra09_family_name(int32_t family, int32_t m);
/* Whether a band pass whose rows hold n_cells cells may take the product-path copy of the band kernel's row tail (1) or runs
 * the generic one (0); a pure host function.  role 1: the column pass, role 0: the row pass (which writes the bitmap);
 * debug != 0: as the debug entry point acx_serra09_debug_pair launches it (eps and, in the row pass, D2 wanted).  A launch
 * takes the copy only if this holds for every pair of it.  The conditions: the wide class (rows of 1018 .. 2041 cells) of
 * the exact arithmetic, pct_mode 0, the inclusive comparison, no debug outputs, and a percentile position (n_cells - 1) kappa
 * that lies at least 2^-8 away from the two ranks around it, the lower of them >= 1, with (upper rank + 2) * 9 <= n_cells.
 * Negative: ACX_ERR_INVALID (the parameters). */
int acx_serra09_fast_tail(const acx_serra09_params *params, int32_t n_cells, int32_t role, int32_t debug);
/* TESTING AND DIAGNOSTICS, not part of the API proper: how many band passes of this process have launched the product-path copy
 * so far (a process-wide counter: every context, every thread) -- what the launcher did, as opposed to what the predicate above
 * says it would do.  The tests observe the dispatch through it; nothing else should depend on it. */
int64_t acx_serra09_fast_tail_launches(void);
/* The same kind of counter for the wide class's per-rotation operand planes: band passes of this process whose kernel read its
 * column operands from the planes (built on the first wide batch of the exact arithmetic, 576 bytes per pooled frame; the
 * environment switch ACX_PLANES=0, read once per process, keeps the class on the rotated pool and this counter where it is). */
int64_t acx_serra09_plane_launches(void);

/* ---- SiMPle (similarity matrix profile) ---------------------------------- */

/*
 * Pool of SiMPle features in f64: `frames` is row-major (sum_i n_i, 12), TIME-major --
 * frame t of track i is the column t of what Simple.load_features(i) returns
 * (simple_silva.py:34-43: WIN/SKIP mean pooling + Hann smoothing + L2 column norm, done by
 * the host).  Independent of the f32 pool of acx_upload_pool.
 */
int acx_upload_pool_f64(acx_ctx *ctx, const double *frames, const int64_t *offsets,
                        int32_t n_tracks, int32_t dim);

/*
 * The same pool from RAW chroma (row-major (sum_i T0_i, 12) f32, C-contiguous per track as
 * deepdish loads it): Simple.load_features on the device for every track at once --
 * n_i = int(T0_i / skip) frames, frame k = mean of raw frames [k skip, k skip + win) clipped to
 * the track (f32, summed in time order like numpy reduces this axis; simple_silva.py:36-41), then
 * smooth(): hann(win_len_smooth + 2, sym) / sum, 'same' convolution along time, L2 norm per
 * frame (simple_silva.py:56-66), in f64.  Defaults of the reference: win 200, skip 100,
 * win_len_smooth 4.  pooled_offsets_out as in acx_upload_raw_pool.
 */
int acx_simple_upload_raw_pool(acx_ctx *ctx, const float *raw, const int64_t *raw_offsets, int32_t n_tracks,
                               int32_t dim, int32_t win, int32_t skip, int32_t win_len_smooth,
                               int64_t *pooled_offsets_out);

/* Copy the f64 pool back (tests): `frames` has room for `capacity` doubles. */
int acx_download_pool_f64(acx_ctx *ctx, double *frames, int64_t capacity);

/*
 * out[k] = -median(matrix profile) of the ORDERED pair (pairs[2k], pairs[2k+1]): OTI of the
 * second track toward the first, then simple_sim -- the value Simple.similarity() stores into
 * Ds['main'][i, j] (simple_silva.py:45-54, 68-126).  f64 like the reference.  sslen = SSLEN
 * (default 10, <= 16); tracks need sslen <= n_i <= 6000 pooled frames.  oti = 0 skips the
 * transposition (Simple.simple_sim alone, simple_silva.py:68).
 */
int acx_simple_pairs(acx_ctx *ctx, const int32_t *pairs, int64_t K, int32_t sslen, int32_t oti,
                     double *out);

/*
 * The matrix profile behind acx_simple_pairs' score, its index, and the matched section (ABI 4, additive).  For the ORDERED
 * pair (q, r) = (pairs[2k], pairs[2k+1]): A = track q (na frames), B' = track r rolled by the OTI shift (nb frames), L = sslen,
 * ma = na - L + 1 rows, mb = nb - L + 1 columns, D[a][b] the distance acx_simple_pairs' kernel computes for that cell (the same
 * operations in the same order).
 *   MP[a]       min over b of D[a][b]
 *   MPI[a]      the SMALLEST b with D[a][b] == MP[a] (the first minimum)
 *   score       -median(MP): the f64 bits acx_simple_pairs returns for the pair;  shift: the OTI shift used (0 with oti = 0)
 *   best_q      the smallest a with MP[a] == min MP;  best_r = MPI[best_q];  best_dist = MP[best_q]
 *   section     the longest maximal run of consecutive rows a0 .. a0 + n - 1 with MPI[a + 1] == MPI[a] + 1 (of several longest
 *               the one with the smallest a0; n >= 1 always: a SiMPle pair always has a match):
 *               q0 = a0, r0 = MPI[a0], q1 = a0 + n - 1, r1 = r0 + n - 1, run_len = n,
 *               q_span = [q0, q1 + L - 1], r_span = [r0, r1 + L - 1]: [first, last] inclusive in pooled frames
 */
typedef struct {
    double score, best_dist;
    int32_t shift, best_q, best_r;
    int32_t q0, r0, q1, r1;
    int32_t q_span[2], r_span[2];
    int32_t run_len;
} acx_simple_alignment;

/*
 * out: K records.  offsets, mp and mpi all NULL: the records alone.  All three given: offsets has K + 1 entries, offsets[0] = 0
 * and offsets[k + 1] - offsets[k] = ma_k; pair k's profile is mp[offsets[k] ..] (f64) and its index mpi[offsets[k] ..] (int32);
 * cap = the number of elements mp and mpi each hold, at least offsets[K]: too small -> ACX_ERR_INVALID with the required number
 * in the message.  Some but not all of the three NULL: ACX_ERR_INVALID.  The whole list is checked before the first launch with
 * the codes of acx_simple_pairs (index out of range ACX_ERR_INVALID, a track shorter than sslen ACX_ERR_SHORT, sslen outside
 * 1..16 or a track above 6000 frames ACX_ERR_UNSUPPORTED, no f64 pool ACX_ERR_STATE).  The pairs run sorted by their second
 * track, in chunks whose device profile buffer stays inside acx_set_scratch_limit (one pair whose profile does not fit:
 * ACX_ERR_NOMEM); results come back in the order of the caller's list.
 */
int acx_simple_profile(acx_ctx *ctx, const int32_t *pairs, int64_t K, int32_t sslen, int32_t oti,
                       acx_simple_alignment *out, int64_t *offsets, double *mp, int32_t *mpi, int64_t cap);

/* ---- EarlyFusion (Tralie 2017) per-pair chain ---------------------------- */

/*
 * Block features of every track, as EarlyFusion.load_features() builds them
 * (earlyfusion_traile.py:100-154): for track i, blocks offsets[i] .. offsets[i+1];
 * mfccs (sum nb, dims[0]=650), ssms (sum nb, dims[1]=1225), chromas (sum nb, dims[2]=480,
 * 40 frames x 12 bins, bin fastest) f32 row-major, chroma_med (n_tracks, 12) f64.
 */
int acx_ef_upload_pool(acx_ctx *ctx, const float *mfccs, const float *ssms, const float *chromas,
                       const double *chroma_med, const int64_t *offsets, int32_t n_tracks,
                       const int32_t *dims);

/*
 * The same pool in slices of whole tracks, for collections whose block features the host cannot (or need
 * not) hold in one piece -- the reference keeps every track's blocks in a Python dict
 * (self.all_block_feats, earlyfusion_traile.py:100-154: 56 GB at DA-TACOS size).
 *   acx_ef_pool_begin   offsets (n_tracks + 1) and dims as in acx_ef_upload_pool; allocates
 *   acx_ef_pool_tracks  tracks [first_track, first_track + count): their rows of the three feature arrays
 *                       and their chroma medians, packed as in acx_ef_upload_pool.  The pointers may be
 *                       HOST or DEVICE memory (features that already live on the GPU, e.g. in a torch
 *                       tensor, are copied device to device).  STREAM CONTRACT: the copy is a blocking
 *                       hipMemcpy(hipMemcpyDefault) ordered against the NULL stream only -- a device source
 *                       written by kernels on another (non-blocking) stream must be COMPLETE before the call:
 *                       synchronise that stream (torch.cuda.synchronize() / hipStreamSynchronize) first.
 *                       Slices may arrive in any order and may be handed over again (the last copy wins)
 *   acx_ef_pool_end     checks that EVERY track was handed over (else ACX_ERR_STATE naming the first missing
 *                       track; the pool stays open, so the missing slices can still be supplied), then the
 *                       non-finite scan, row norms, the GEMM operands (two fp16 or three bf16 terms per value, acx_set_ef_gemm); the pool is usable from here on
 */
int acx_ef_pool_begin(acx_ctx *ctx, const int64_t *offsets, int32_t n_tracks, const int32_t *dims);
int acx_ef_pool_tracks(acx_ctx *ctx, int32_t first_track, int32_t count, const float *mfccs, const float *ssms,
                       const float *chromas, const double *chroma_med);
int acx_ef_pool_end(acx_ctx *ctx);

/* Block-feature parameters of EarlyFusion.load_features (ctor arguments blocksize,
 * mfccs_per_block, chromas_per_block; earlyfusion_traile.py:44-45): defaults 20, 50, 40. */
typedef struct {
    int32_t blocksize;          /* beats per block                                  */
    int32_t mfccs_per_block;    /* rows an MFCC block is resized to   (<= 64)        */
    int32_t chromas_per_block;  /* rows a chroma block is resized to  (<= 64)        */
} acx_ef_prep_params;

/*
 * EarlyFusion.load_features(i) for ONE track on the device (earlyfusion_traile.py:100-140, with
 * resize_block :214-247): from the track's chroma (n_chroma, 12) f32, MFCCs (n_mfcc, ncoef) f32
 * TIME-major (feats['mfcc_htk'].T; NaN -> 0 as at :108) and beat onsets (frame indices), the
 * n_blocks = n_beats - blocksize block features
 *   mfccs (n_blocks, mfccs_per_block * ncoef), ssms (n_blocks, mfccs_per_block (mfccs_per_block - 1) / 2),
 *   chromas (n_blocks, chromas_per_block * 12)  f32 row-major, chroma_med (12) f64
 * into host buffers (any may be NULL).  The anti-aliased resize restates skimage.transform.resize
 * (see acoss_amd/csrc/ef_prep_kernels.hpp; unpinned: skimage is absent from the reference's tree).
 * Refused before anything is allocated (here and in acx_ef_upload_raw_pool, whose pool then stays as it is):
 * a negative onset -> ACX_ERR_INVALID naming the track (numpy's slice would count it from the end); a block
 * whose resize needs a Gaussian of radius int(4 sigma + 0.5) > 512, sigma = (frames / rows - 1) / 2, i.e. of
 * more than about 257 frames per row -> ACX_ERR_UNSUPPORTED naming the track and the block.
 */
int acx_ef_block_features(acx_ctx *ctx, const float *chroma, int64_t n_chroma, const float *mfcc, int64_t n_mfcc,
                          int32_t ncoef, const int64_t *onsets, int32_t n_beats, const acx_ef_prep_params *prep,
                          float *mfccs, float *ssms, float *chromas, double *chroma_med);

/*
 * The block-feature pool of a whole collection built on the device and kept there: the same as
 * acx_ef_block_features for every track followed by acx_ef_upload_pool, without the features
 * ever visiting the host.  chroma (sum n_chroma_i, 12), mfcc (sum n_mfcc_i, ncoef), onsets
 * (sum n_beats_i) packed, track i at *_offsets[i] .. *_offsets[i+1].  block_offsets_out
 * (n_tracks + 1, may be NULL) receives the block offsets.  Tracks with fewer than blocksize + 1
 * beats have no block.
 */
int acx_ef_upload_raw_pool(acx_ctx *ctx, const float *chroma, const int64_t *chroma_offsets, const float *mfcc,
                           const int64_t *mfcc_offsets, int32_t ncoef, const int64_t *onsets,
                           const int64_t *onset_offsets, int32_t n_tracks, const acx_ef_prep_params *prep,
                           int64_t *block_offsets_out);

/*
 * The block-feature pool read back as the device holds it (host-side copies only; tests and inspection):
 * mfccs (n_blocks, dims[0]), ssms (n_blocks, dims[1]), chromas (n_blocks, dims[2]) -- the chroma rows are
 * ALREADY unit-normalised (a row of zeros stays zero) --, mfcc_sq / ssm_sq (n_blocks) the squared row norms
 * of the two Euclidean features, chroma_med (n_tracks, 12), offsets (n_tracks + 1) the block offsets,
 * *n_tracks and dims[3].  Any pointer may be NULL (a first call may ask for *n_tracks and dims alone, a
 * second for the offsets).  No finished pool (none uploaded, or one still open): ACX_ERR_STATE.
 */
int acx_ef_download_pool(acx_ctx *ctx, float *mfccs, float *ssms, float *chromas, float *mfcc_sq, float *ssm_sq,
                         double *chroma_med, int64_t *offsets, int32_t *n_tracks, int32_t *dims);

typedef struct {
    double kappa;     /* csm_to_binary neighbourhood (EarlyFusion ctor kappa = 0.1)  */
    int32_t K;        /* getWCSM neighbours (ctor K = 10)                            */
} acx_ef_params;

/*
 * out[4k .. 4k+3] = Smith-Waterman scores (mfccs, ssms, chromas, early) of pair
 * (pairs[2k], pairs[2k+1]) -- what EarlyFusion.similarity() stores into
 * Ds['mfccs'|'ssms'|'chromas'|'early'][i, j] (earlyfusion_traile.py:157-198).
 */
int acx_earlyfusion_pairs(acx_ctx *ctx, const int32_t *pairs, int64_t K, const acx_ef_params *params,
                          float *out);

/*
 * Arithmetic of the three cross-similarity products (mfccs, ssms: get_csm, cross_recurrence.py:30-48; chromas:
 * get_csm_blocked_oti, :105-134 -- the reference's are BLAS sgemms in f32).  The matrix-pipe modes lay the pairs of a
 * batch out as dense rectangles (query tracks' blocks x reference tracks' blocks), so that the 256 x 128 tiles of the
 * GEMM are full and a track is read once per rectangle; chroma rows are kept bin-major, which turns the OTI roll into a
 * shift of the row by whole 16-byte pieces (blocks of a multiple of 8 frames; others: f32 MFMAs).
 *   ACX_EF_GEMM_F16X2 (default)   every value as TWO fp16 terms of x / s, s = the power of two that puts the largest
 *                                 |x| of the value's own ROW into [2^14, 2^15) (so a track's operands depend on the
 *                                 track alone); three fp16 MFMAs per cell and 32 k -- x1 y2, x2 y1, x1 y1, f32
 *                                 accumulation; x2 y2 (<= 2^-22 |x y|) stays below the accumulator's rounding and is
 *                                 not formed -- and the product rescaled by s_row s_column (exact).  An
 *                                 operand keeps 22 of its 24 significant bits: a relative rounding of 2^-23 per
 *                                 value, below the accumulation error of any f32 sgemm over K = 480 .. 1225.
 *   ACX_EF_GEMM_BF16X3            three-term bf16 splits (all 24 bits of every value), six bf16 MFMAs per cell and
 *                                 32 k: the dropped terms are below one f32 rounding of the product.  1.27 x the GEMM
 *                                 time of the default (round 3's default)
 *   ACX_EF_GEMM_F32               f32 MFMA (v_mfma_f32_16x16x4_f32: exact f32 products, f32 accumulation), one
 *                                 matrix at a time
 *   ACX_EF_GEMM_BF16X3_CHROMA_F32 the rectangles of BF16X3, chroma by f32 MFMAs (round 3's first kernel)
 * All meet the same bound against the f64 truth (tests/test_gpu_earlyfusion.py) and move as many scores against
 * f64-evaluated matrices as the reference's own f32 arithmetic does (tests/test_gpu_parity_sets.py, 124 750 pairs;
 * profiles/r04_parity_ef.json); scores that differ between them sit on a row-kappa threshold tie.  The split pool
 * holds ONE operand format (46 GB of fp16 terms or 69 GB of bf16 terms at DA-TACOS size, in one allocation sized for the larger):
 * changing between F16X2 and the bf16 modes re-splits the pool
 * on the next call.  mode -1 = the default.
 */
enum { ACX_EF_GEMM_BF16X3 = 0, ACX_EF_GEMM_F32 = 1,
       ACX_EF_GEMM_BF16X3_PAIRWISE = 2, /* mfccs / ssms in BF16X3's arithmetic, one matrix at a time (round 2's
                                           kernel; bit-identical matrices -- kept as the cross-check of the rectangle
                                           kernel), chroma by f32 MFMAs */
       ACX_EF_GEMM_BF16X3_CHROMA_F32 = 3, ACX_EF_GEMM_F16X2 = 4, ACX_EF_GEMM_DEFAULT = ACX_EF_GEMM_F16X2 };
int acx_set_ef_gemm(acx_ctx *ctx, int32_t mode);

/*
 * Arithmetic of getWCSM's kernel weights and of the fused matrix exp(-(W_mfcc + W_ssm + W_chroma)) (similarity_fusion.py:38-54,
 * earlyfusion_traile.py:176-183).  The fused matrix is only RANKED (csm_to_binary) afterwards.
 *   ACX_EF_FUSE_FAST (default)  exp(-C^2 / (2 (eps / 2)^2)) = exp2(-18 log2(e) (C / (r + c + C))^2): one v_rcp_f32, one v_exp_f32
 *                               per weight (about 1e-6 relative against the reference's numpy f32)
 *   ACX_EF_FUSE_EXACT           the reference's own operation order in f32 with IEEE divisions and expf (~12 x the instructions):
 *                               differs from numpy by the last bit of the exponentials only, so that a regression in the
 *                               selection / alignment kernels can be told from an approximation tie
 */
enum { ACX_EF_FUSE_FAST = 0, ACX_EF_FUSE_EXACT = 1 };
int acx_set_ef_fuse(acx_ctx *ctx, int32_t mode);

/* One pair with intermediates (tests): csm (3, M, N), fused (M, N), scores (4); any may be NULL. */
int acx_ef_debug_pair(acx_ctx *ctx, int32_t i, int32_t j, const acx_ef_params *params,
                      float *csm, float *fused, float *scores, int32_t *oti);

/* The same intermediates for pair `which` of a LIST of K pairs that runs as ONE batch (tests, ABI 4): the list goes through the
 * rectangle GEMM the way acx_earlyfusion_pairs sends it -- many pairs per workgroup tile, shared operands, sub-tiles dropped
 * into their own pairs' matrices -- so that a cell of a multi-pair rectangle can be held against an f64 product, not only the
 * one-pair rectangle of acx_ef_debug_pair.  scores: (K, 4), all pairs.  A list that needs more than one batch (65 535 pairs or
 * the scratch limit): ACX_ERR_UNSUPPORTED. */
int acx_ef_debug_pairs(acx_ctx *ctx, const int32_t *pairs, int64_t K, const acx_ef_params *params, int64_t which,
                       float *csm, float *fused, float *scores, int32_t *oti);

/* What the EarlyFusion back end leaves behind for pair `which` of a SORTED list of K pairs that runs as ONE batch (tests): the
 * call acx_earlyfusion_pairs makes for that list -- the fused matrix made and binarised in registers, never stored, the same
 * kernel choices -- and then, copied from the device:
 *   bits  (4, M, pitch / 32) uint32, pitch = N rounded up to 64: the binarised matrices (mfccs, ssms, chromas, fused) as the
 *         selection kernels wrote them, bit j % 32 of word j / 32 = B[i][j], pad bits 0
 *   t     (4, M) thresholds, jcut (4, M) tie columns: B_ij = C_ij < t_i, or C_ij == t_i and j <= jcut_i (0x7fffffff: every tie)
 *   r     (3, M) row and c (3, N) column neighbourhood means of getWCSM (similarity_fusion.py:38-54)
 *   scores (K, 4), all pairs.
 * Any output may be NULL.  A list with a track of more than 1024 blocks takes the float-matrix kernels and leaves no bitmaps:
 * `bits` must then be NULL (else ACX_ERR_INVALID); the vectors are returned all the same.  An unsorted list: ACX_ERR_INVALID;
 * a list that needs more than one batch: ACX_ERR_UNSUPPORTED, before any launch (acx_ef_debug_pairs likewise). */
int acx_ef_debug_bits(acx_ctx *ctx, const int32_t *pairs, int64_t K, const acx_ef_params *params, int64_t which,
                      uint32_t *bits, float *t, int32_t *jcut, float *r, float *c, float *scores);

/*
 * The batch plan of a pair list, for tests and tools -- no context, no device: what acx_earlyfusion_pairs would do with the
 * list on a pool whose tracks have these block counts, told by the functions the run itself calls
 * (acoss_amd/csrc/ef_plan.hpp; the per-process switch ACX_EF_ROWSTAT2 applies).
 *   blocks        blocks per track, as uploaded (n_tracks of them)
 *   scratch_limit bytes, as acx_set_scratch_limit; <= 0: the default without a device -- env ACX_SCRATCH_GB, else unbounded
 *                 (a context's default is 40 % of ITS device's memory, at most 36 GB)
 *   keep_fused    != 0: as the debug entries that return the fused matrix run the list (acx_ef_debug_pair / _pairs): it is stored
 *   out           K records, in the order of `pairs`:
 *     M, N        blocks of the pair's tracks (rows, columns of its matrices); kbin: csm_to_binary's neighbours per row
 *     batch       the batch the pair runs in; run_pos: its position in run order (sorted by first track, second track --
 *                 batches are contiguous runs of THAT order)
 *     path        0: the bit path, 1: the float path (a track of more than 1024 blocks anywhere in the list)
 *     row_kernel, col_kernel, fuse_kernel, sw_kernel   ACX_EF_ROW_* / _COL_* / _FUSE_* / _SW_* of its batch
 *     need        floats of the scratch arena the pair takes
 * A list the run would refuse returns the run's code for it (ACX_ERR_INVALID: an index, or the parameters; ACX_ERR_SHORT: a
 * track without blocks; ACX_ERR_NOMEM: a pair beyond the scratch limit) and fills nothing; the message: acx_last_error(NULL).
 */
enum { ACX_EF_ROW_TWO = 0,      /* ef_rowstat2_kernel: two rows per wave, rows of <= 512 cells                      */
       ACX_EF_ROW_2 = 1,        /* ef_rowstat_kernel<2, false>: 8 values per lane, <= 512 cells                     */
       ACX_EF_ROW_4 = 2,        /* ef_rowstat_kernel<4, false>: 16 values per lane, <= 1024 cells                   */
       ACX_EF_ROW_LONG = 3 };   /* ef_rowstat_long_kernel: any length                                               */
enum { ACX_EF_COL_ROWPASS = 0,  /* the row kernel on the transposed matrices (K > 16)                               */
       ACX_EF_COL_10 = 1,       /* ef_colstat_kernel<10> (K <= 10)                                                  */
       ACX_EF_COL_16 = 2,       /* ef_colstat_kernel<16>                                                            */
       ACX_EF_COL_NONE = 3 };   /* a caller's matrix has no column statistics (never in this report)                */
enum { ACX_EF_FUSE_NARROW = 0,  /* ef_rowstat_kernel<2, true>: fused matrix made and binarised in registers         */
       ACX_EF_FUSE_WIDE = 1,    /* ef_rowstat_kernel<4, true>                                                       */
       ACX_EF_FUSE_FLOAT = 2,   /* ef_fuse_kernel stores it; the one-row kernel of row_kernel's class selects on it */
       ACX_EF_FUSE_NONE = 3 };  /* a caller's matrix is not fused (never in this report)                            */
enum { ACX_EF_SW_H16_8 = 0,     /* sw_bits_h16_kernel<8>: bitmaps, rows of <= 512 cells                             */
       ACX_EF_SW_H16_16 = 1,    /* sw_bits_h16_kernel<16>: <= 1024 cells                                            */
       ACX_EF_SW_8 = 2,         /* sw_kernel<8>: float matrices, <= 512 cells                                       */
       ACX_EF_SW_16 = 3,        /* sw_kernel<16>: <= 1024 cells                                                     */
       ACX_EF_SW_LONG = 4 };    /* sw_long_kernel: any length                                                       */
typedef struct acx_ef_plan_rec {
    int32_t M, N, kbin;
    int32_t batch;
    int32_t path;
    int32_t row_kernel, col_kernel, fuse_kernel, sw_kernel;
    int32_t reserved;
    int64_t run_pos;
    int64_t need;
} acx_ef_plan_rec;
int acx_ef_plan(const int64_t *blocks, int32_t n_tracks, const int32_t *pairs, int64_t K, const acx_ef_params *params,
                int64_t scratch_limit, int32_t keep_fused, acx_ef_plan_rec *out);
/* Printable name of a kernel of the report: stage 0..3 (row statistics, column statistics, fused selection, Smith-Waterman) and
 * the enum's value; NULL for an unknown one.  The string is static. */
const char *acx_ef_kernel_name(int32_t stage, int32_t kernel);

/* The run of acx_csm_binary_sw for one (M, N) f32 matrix with the caller's neighbourhood size K, and what it left behind (tests):
 * bits (M, pitch / 32), t (M), jcut (M), r (M) as above, and the Smith-Waterman score.  Any output may be NULL; M or N above 1024:
 * `bits` must be NULL. */
int acx_csm_debug_bits(acx_ctx *ctx, const float *D, int32_t M, int32_t N, double kappa, int32_t K,
                       uint32_t *bits, float *t, int32_t *jcut, float *r, float *score);

/* csm_to_binary(D, kappa) (cross_recurrence.py:136-161: exactly k = round(kappa N) cells per row;
 * ties at the k-th value are taken in column order) followed by smith_waterman_constrained, for
 * one (M, N) f32 matrix -- the tail of every feature's chain in earlyfusion_traile.py:165-197
 * (tests). */
int acx_csm_binary_sw(acx_ctx *ctx, const float *D, int32_t M, int32_t N, double kappa, float *score);

/* smith_waterman_constrained (alignment_tools.py:26-46) of one binary (M, N) uint8 matrix on
 * the device DP (tests against the reference goldens).  Non-{0,1} input -> ACX_ERR_INVALID
 * (the reference raises IOError). */
int acx_sw_binary(acx_ctx *ctx, const uint8_t *B, int32_t M, int32_t N, float *score);

/* The same on the BIT kernel every ordinary EarlyFusion call runs (tests): B is packed on the host into the layout of the
 * binarised matrices (see acx_ef_debug_bits) and aligned by the packed 16-bit Smith-Waterman, N <= 512 and N <= 1024 columns
 * in the variants the product launches.  M or N above 1024: ACX_ERR_INVALID; non-{0,1} input as acx_sw_binary. */
int acx_sw_bits_binary(acx_ctx *ctx, const uint8_t *B, int32_t M, int32_t N, float *score);

/* WHERE the constrained Smith-Waterman alignment of every listed pair lies in ONE of the four binarised matrices, and optionally its
 * path (ABI 4, additive).  plane: 0 mfccs, 1 ssms, 2 chromas, 3 early (the fused matrix).  With T[i][j] = S[i+1][j+1] of
 * smith_waterman_constrained (alignment_tools.py:26-46), in integer tenths,
 *   T[i][j] = max(0, (B[i][j] ? 10 : -10) + max(U[i-1][j-1], U[i-2][j-1], U[i-1][j-2])),  U = T + (B ? 0 : -7),
 * T = 0 in rows and columns 0, 1, and only the cells 2 <= i <= M-2, 2 <= j <= N-2 count.  Everything is reported in this T frame:
 * rows are block indices of the query (pairs[2 k]), columns block indices of the reference (pairs[2 k + 1]).
 *   out[k].score     max T / 10: the bits acx_earlyfusion_pairs returns for that ordered pair and plane
 *   (q1, r1)         the end: the counted cell, first in row-major order, at which T attains the maximum
 *   (q0, r0)         the start: follow predecessors from the end -- the predecessor of a cell with T > 0 is the first of
 *                    (i-1, j-1), (i-2, j-1), (i-1, j-2) whose U equals the maximum of the three -- to the last cell with T > 0
 *   no match         (score 0; M < 4 or N < 4): the four coordinates are -1
 *   path_off, cells  both NULL: the records alone.  Both given: pair k's path is cells[2 path_off[k] .. 2 path_off[k + 1]), the
 *                    (q, r) of every cell from the start to the end, both included; consecutive cells differ by (1, 1), (2, 1) or
 *                    (1, 2); a pair without a match has none.  Exactly one of the two NULL: ACX_ERR_INVALID.
 *   cap              cells the buffer holds: at least the sum of min(M_k, N_k) over the list, checked before the first launch;
 *                    too small -> ACX_ERR_INVALID with the required number in the message
 * Results come back in the order of the caller's list (the run sorts it as acx_earlyfusion_pairs does).  The whole list is checked
 * before the first launch: a track of more than 1024 blocks anywhere in it -> ACX_ERR_UNSUPPORTED ("alignment needs the bit
 * path: at most 1024 blocks"); plane outside 0..3 -> ACX_ERR_INVALID; an index out of range, a track without blocks, no pool:
 * the codes and messages of acx_earlyfusion_pairs.  A failed call leaves nothing in flight, and a valid call after it succeeds. */
int acx_ef_align(acx_ctx *ctx, const int32_t *pairs, int64_t K, const acx_ef_params *params, int32_t plane /* 0..3 */,
                 acx_alignment *out /* K */, int64_t *path_off /* K + 1 or NULL */, int32_t *cells /* cap x 2 or NULL */, int64_t cap);

/* The same DP alone on a caller's binary (M, N) uint8 plot (tests), packed on the host as acx_sw_bits_binary packs it.  cells and
 * n_cells both NULL: the record alone; both given: cap >= min(M, N) (else ACX_ERR_INVALID, nothing launched), the path goes to
 * cells (cap x 2 int32) from the start to the end and *n_cells is its length.  M or N above 1024: ACX_ERR_UNSUPPORTED; a value
 * above 1 in B: ACX_ERR_INVALID. */
int acx_sw_align_binary(acx_ctx *ctx, const uint8_t *B, int32_t M, int32_t N, acx_alignment *out, int32_t *cells, int64_t cap,
                        int64_t *n_cells);

/* acx_ef_align for tracks of ANY length (ABI 4, additive): the same arguments, contract, cap rule, sort and output order, without the
 * refusal of tracks of more than 1024 blocks.  A list without such a track runs exactly as acx_ef_align runs it.  Any other list takes
 * the float path of acx_earlyfusion_pairs, and the alignment of ALL its pairs, short ones included, is read off the float matrices,
 * row thresholds and tie columns that path leaves on the device, in strips of 1024 columns: B[i][j] = C[i][j] < t_i, or
 * C[i][j] == t_i and j <= jcut_i (the plot the scores of that path are taken from; out[k].score has their bits).  The whole list is
 * checked before the first launch: the codes and messages of acx_ef_align minus the length refusal; a pair that does not fit the
 * scratch limit -> ACX_ERR_NOMEM, as in acx_earlyfusion_pairs.  A failed call leaves nothing in flight, and a valid call after it
 * succeeds. */
int acx_ef_align_long(acx_ctx *ctx, const int32_t *pairs, int64_t K, const acx_ef_params *params, int32_t plane /* 0..3 */,
                      acx_alignment *out /* K */, int64_t *path_off /* K + 1 or NULL */, int32_t *cells /* cap x 2 or NULL */, int64_t cap);

/* The strip-wise DP alone on a caller's binary (M, N) uint8 plot of any size (tests), set up as acx_sw_binary sets up its long case
 * (the plot as a 0 / 1 float matrix, thresholds 0).  The arguments of acx_sw_align_binary; every size, 4 x 4 included, runs the kernel
 * of acx_ef_align_long's float path.  A value above 1 in B: ACX_ERR_INVALID. */
int acx_sw_align_long_binary(acx_ctx *ctx, const uint8_t *B, int32_t M, int32_t N, acx_alignment *out, int32_t *cells, int64_t cap,
                             int64_t *n_cells);

/* EVERY matched section of every listed pair in ONE binarised matrix, not only the best alignment (ABI 4, additive).  pairs, params,
 * plane, the T frame, score, end, predecessor, start and path: acx_ef_align's.  opts: the acx_section_opts of
 * acx_serra09_align_sections with the same checks (max_sections S in 1..16, min_score > 1, min_ratio in 0..1, pad >= 0; else
 * ACX_ERR_INVALID).
 *   section 0       acx_ef_align's record for that pair and plane, bit for bit, reported iff its score >= min_score; otherwise the
 *                   pair has no sections
 *   free intervals  the rows start as one free interval [0, M - 1]; a section with rows q0..q1 inside the free interval [a, b]
 *                   EXCLUDES [max(a, q0 - pad), min(b, q1 + pad)], and [a, b] is replaced by what is left above and below
 *   section k + 1   the alignment of T', the same recursion with T' = 0 on every cell of an excluded row -- U' = (B ? 0 : -7) there,
 *                   what rows 0 and 1 hold: no alignment runs through an excluded stretch.  Reported iff its f32 score >=
 *                   max(min_score, min_ratio * score_0) (one f32 multiply, equality counts); the search ends at the first section
 *                   that fails, or after S
 * Scores do not increase with k, the row ranges [q0, q1] of a pair's sections are pairwise disjoint, reference columns may be
 * shared, and max_sections = 1 is acx_ef_align.
 *   out             K x S records, pair k's from out[k * S], section 0 first; behind its n_sections[k] sections the no-match record
 *   path_off, cells both NULL: the records alone.  Both given: path_off has K * S + 1 entries, record t = k * S + s has the cells
 *                   cells[2 path_off[t] .. 2 path_off[t + 1]) from its start to its end.  Exactly one NULL: ACX_ERR_INVALID.
 *   cap             at least the sum of min(M_k, S * min(M_k, N_k)) over the list, checked before the first launch; too small ->
 *                   ACX_ERR_INVALID with the required number in the message
 * Tracks of at most 1024 blocks: a longer one anywhere in the list -> ACX_ERR_UNSUPPORTED for the whole list before any launch, as
 * acx_ef_align refuses it.  Every other check, code and message of the list: acx_ef_align's.  A failed call leaves nothing in flight,
 * and a valid call after it succeeds. */
int acx_ef_align_sections(acx_ctx *ctx, const int32_t *pairs, int64_t K, const acx_ef_params *params, int32_t plane /* 0..3 */,
                          const acx_section_opts *opts, acx_alignment *out /* K x max_sections */, int32_t *n_sections /* K */,
                          int64_t *path_off /* K x max_sections + 1, or NULL */, int32_t *cells /* cap x 2, or NULL */, int64_t cap);

/* The same DP alone on a caller's binary (M, N) uint8 plot (tests), packed as acx_sw_align_binary packs it: out holds max_sections
 * records, *n_sections their number, path_off (max_sections + 1) and cells as above with cap >= min(M, max_sections * min(M, N)).
 * M or N above 1024: ACX_ERR_UNSUPPORTED; a value above 1 in B: ACX_ERR_INVALID; nothing is launched then. */
int acx_sw_sections_binary(acx_ctx *ctx, const uint8_t *B, int32_t M, int32_t N, const acx_section_opts *opts,
                           acx_alignment *out, int32_t *n_sections, int64_t *path_off, int32_t *cells, int64_t cap);

/* ---- FTM2D (2D Fourier transform magnitudes, Bertin-Mahieux & Ellis) ------ */

/* Constructor arguments of FTM2D (ftm2d.py:23): defaults PWR 1.96, WIN 75, C 5. */
typedef struct {
    double pwr;         /* chrompwr exponent (ftm2d.py:58)                                        */
    double c;           /* log(C x + 1) compression of every window (:61)                         */
    int32_t win;        /* beats per window (:60); 1..256 on the device                           */
    int32_t reserved;   /* 0                                                                      */
} acx_ftm2d_params;

void acx_ftm2d_default_params(acx_ftm2d_params *p);

/*
 * The shingle pool of a collection -- FTM2D.load_features(i) for every track (ftm2d.py:38-64) -- built on the device
 * from raw features streamed in batches of whole tracks, so that the host never holds the collection's chroma at once
 * (the reference keeps only the shingles, self.shingles, :29):
 *   acx_ftm2d_pool_begin   allocates an (n_tracks, 12 WIN) f64 pool for `params` (copied)
 *   acx_ftm2d_pool_tracks  tracks [first_track, first_track + count): chroma (sum T_i, 12) f32 as loaded
 *                          (feats[chroma_type]), track i at rows chroma_offsets[i] .. chroma_offsets[i + 1]; beat onsets
 *                          (frame indices, feats['madmom_features']['onsets'], :55) at onset_offsets[i] .. [i + 1] --
 *                          the packed layout of acx_ef_upload_raw_pool, offsets (count + 1) index into the arrays given.
 *                          Per track: librosa.util.sync(X.T, onsets, aggregate=np.median) (onsets clipped to [0, T],
 *                          0 and T added, np.unique; f32 median per bin and segment, bit-identical to np.median),
 *                          chrompwr, |fft2| of every WIN-beat window in fftshift order as WIN-point DFTs of the 7
 *                          chroma-DFT rows (rows 7..11 by conjugate symmetry), window L2 norm, log(C x + 1), exact f64
 *                          median over the windows, final L2 norm -- f64 from the synced f32 values.  The WHOLE batch is
 *                          checked first: a negative onset or fewer than WIN beats fails with ACX_ERR_INVALID naming the
 *                          first such track and nothing is launched (the reference raises / returns None there, :60,
 *                          :130); NaN / Inf chroma follows the context's non-finite policy.  The window matrices run in
 *                          sub-batches under acx_set_scratch_limit.  Slices may come in any order and again (last wins)
 *   acx_ftm2d_pool_end     checks that every track was handed over (else ACX_ERR_STATE naming the first missing one;
 *                          the pool stays open); the pool is usable from here on
 * A track whose shingle median is all zero (silent chroma) gets NaN, as in the reference (:63).
 */
int acx_ftm2d_pool_begin(acx_ctx *ctx, int32_t n_tracks, const acx_ftm2d_params *params);
int acx_ftm2d_pool_tracks(acx_ctx *ctx, int32_t first_track, int32_t count, const float *chroma, const int64_t *chroma_offsets,
                          const int64_t *onsets, const int64_t *onset_offsets);
int acx_ftm2d_pool_end(acx_ctx *ctx);

/* Ready shingles instead (synthetic benchmarks, FTM2D.set_features): (n_tracks, dim) f64 row-major, any dim >= 1.
 * Replaces the pool. */
int acx_ftm2d_upload_shingles(acx_ctx *ctx, const double *shingles, int32_t n_tracks, int32_t dim);
/* Copy the shingle pool back: `shingles` has room for `capacity` doubles (n_tracks x dim needed). */
int acx_ftm2d_download_shingles(acx_ctx *ctx, double *shingles, int64_t capacity);

/*
 * One track through the same kernels with every intermediate (tests; the pool is not touched).  dims[3] =
 * {nbeats, nwin = nbeats - WIN + 1, D = 12 WIN} is always written, so a call with every output NULL asks for the
 * shape.  Outputs (any may be NULL): synced (nbeats, 12) f32 -- the beat-synchronous chroma, TIME-major (hpcp.T of
 * ftm2d.py:56); pwr (nbeats, 12) f64 -- chrompwr (:58), time-major; logwin (nwin, D) f64 -- log(C |fft2| / norm + 1)
 * of every window (:60-61); median (D) f64 -- before the final norm (:62); shingle (D) f64 (:63).
 */
int acx_ftm2d_debug_track(acx_ctx *ctx, const float *chroma, int64_t n_frames, const int64_t *onsets, int64_t n_onsets,
                          const acx_ftm2d_params *params, float *synced, double *pwr, double *logwin, double *median,
                          double *shingle, int64_t *dims);

/*
 * out[k] = exp(-sum((s_i - s_j)^2)) for pair (i, j) = (pairs[2k], pairs[2k+1]) -- the value FTM2D.similarity() stores
 * into the float32 Ds['main'][i, j] (ftm2d.py:85-97): the sum in f64 over the dimensions in order (difference form,
 * no cancellation), exp in f64, rounded to f32.  i == j gives 1.  The whole list is checked before the first launch.
 */
int acx_ftm2d_pairs(acx_ctx *ctx, const int32_t *pairs, int64_t K, float *out);

/* ---- late fusion (N x N post-step) ---------------------------------------- */

/*
 * Similarity network fusion of m affinity matrices: the cross-diffusion loop of
 * doSimilarityFusionWs (similarity_fusion.py:146-186; EarlyFusion.do_late_fusion,
 * earlyfusion_traile.py:200-206; LateFusionChen.do_late_fusion) in f64 on the device.
 *   Ws[i]  (n, n) f64 row-major affinity matrix W_i (getW, :15-36 -- prepared by the host)
 *   Js[i]  (n, K) int32, Vs[i] (n, K) f64: the row-normalised K-nearest-neighbour kernel S_i of
 *          W_i (getS, :124-144) as K (column, weight) pairs per row
 *   out    (n, n) f64: the fused matrix, mean of the P_i after `niters` sweeps
 * P_i starts as the row-normalised W_i (getP, :101-122); per sweep and matrix
 * P_i <- S_i mean_{k != i}(P_k) S_i^T + reg_diag I, where from the second sweep on a matrix updated
 * earlier in the sweep is already seen by the later ones, as in the reference (:179).
 * 2 <= m <= 8.  Device memory: (2 m + 2) n^2 doubles.
 */
int acx_snf_fuse(acx_ctx *ctx, const double *const *Ws, const int32_t *const *Js, const double *const *Vs,
                 int32_t m, int32_t n, int32_t K, int32_t niters, double reg_diag, double *out);

/*
 * The whole of doSimilarityFusion (similarity_fusion.py:188-196) on the device: from m distance
 * matrices Ds[i] (n, n) f64 row-major -- getW (:15-36: symmetrise, zero diagonal, local scale =
 * mean of the K + 1 smallest of a row x (K + 1) / K, W = exp(-D^2 / (2 (mu eps)^2))), the kNN
 * kernels (getS, ties at the cut in column order), getP and the cross-diffusion loop as in
 * acx_snf_fuse.  out (n, n) f64: the fused matrix; Ws_out (may be NULL, entries may be NULL): the m
 * affinity matrices.  K <= 64.
 */
int acx_snf_fuse_dists(acx_ctx *ctx, const double *const *Ds, int32_t m, int32_t n, int32_t K, int32_t niters,
                       double reg_diag, double mu, double *out, double *const *Ws_out);

/*
 * What the kernels of acx_snf_fuse_dists leave behind for ONE matrix (tests): the same host function launches them for
 * the product and for this call.  M (n, n) f64 row-major.  from_stage = 0: M is a distance matrix, all five kernels
 * run; from_stage = 1: M is already an affinity matrix, only the neighbour lists and the row normalisation run on it
 * (S and md are not written).  Outputs, any may be NULL: S (n, n) the symmetrised matrix with its zero diagonal,
 * md (n) the local scale, W (n, n) the affinity matrix, J (n, K) int32 / V (n, K) the kNN kernel, P (n, n) the
 * row-normalised W.  1 <= K <= min(n, 64).  J and V are filled with -1 / NaN before the launch: a slot that no lane
 * wrote shows as such.
 */
int acx_snf_debug_stages(acx_ctx *ctx, const double *M, int32_t n, int32_t K, double mu, int32_t from_stage,
                         double *S, double *md, double *W, int32_t *J, double *V, double *P);

/*
 * ONE update of the cross-diffusion loop as acx_snf_fuse launches it (tests; the same host function):
 * acc = (srcs[0] + ... + srcs[m_src - 1]) * scale, UT = acc S^T, P = S UT + reg_diag I, with S = (J, V) (n, K) as in
 * acx_snf_fuse, any 1 <= K <= n, 1 <= m_src <= 8.  variant: 0 = the gather kernel the product chooses for this n,
 * 1 = the row of acc in LDS (ACX_ERR_UNSUPPORTED when n doubles do not fit; refused before any array is read),
 * 2 = gathers from global memory.  Only the rows `rows[0 .. n_rows)` are copied back: acc_rows, ut_rows, p_rows
 * (n_rows, n) f64, any may be NULL.
 */
int acx_snf_debug_update(acx_ctx *ctx, const double *const *srcs, int32_t m_src, int32_t n, int32_t K, double scale,
                         const int32_t *J, const double *V, double reg_diag, int32_t variant, const int32_t *rows,
                         int32_t n_rows, double *acc_rows, double *ut_rows, double *p_rows);

/* ---- EarlyFusion: the full cross-diffusion fusion for listed pairs ---------- */

/*
 * The early fusion of Tralie's ISMIR 2017 paper, the "Step 3" that earlyfusion_traile.py:142-148 disables, for ordered
 * pairs of the uploaded EarlyFusion pool.  Per pair (A of M blocks, B of N, n = M + N) and per feature (mfccs, ssms,
 * chromas): W = getWCSMSSM(S^A, S^B, C, K, mu = 0.5) (similarity_fusion.py:76-99) from the f32 matrices of the pairs
 * (A, A), (B, B), (A, B) under the current acx_set_ef_gemm mode, in f64; D = doSimilarityFusionWs of the three W
 * (:146-186; params->K neighbours, niters sweeps); X = D[0:M, M:] + D[M:, 0:M]^T; row i of the plot holds the
 * round(kappa N) columns with the largest X[i, :] (csm_to_binary(exp(-X), kappa) without the exponential; ties at the
 * cut in column order); out[k] = smith_waterman_constrained of the plot (alignment_tools.py:26-46), one f32 per pair in
 * the caller's order.  The stages restate reference functions; the composition is the method's, not the reference's.
 * The whole list is checked before the first launch.  ACX_ERR_UNSUPPORTED: a pair with k1 = int(K M / (M + N)) < 1,
 * k2 = K - k1 < 1, k1 + 1 >= M or k2 + 1 >= N (np.partition raises or divides by zero there; the message names the
 * pair's position), a track of more than 1024 blocks, K > 64.  ACX_ERR_INVALID: niters < 1.  Indices, tracks without
 * blocks and a missing pool: as acx_earlyfusion_pairs.
 */
int acx_ef_crossfusion_pairs(acx_ctx *ctx, const int32_t *pairs, int64_t K_pairs, const acx_ef_params *params,
                             int32_t niters, double reg_diag, float *out);

/*
 * ONE pair of the pool through the same host function, every intermediate copied back (tests; any output may be NULL):
 * ssm_a (3, M, M), ssm_b (3, N, N), csm (3, M, N) f32; W (3, n, n), D (n, n), X (M, N) f64; bits (M, pitch / 32) uint32,
 * pitch = N rounded up to 64, bit j % 32 of word j / 32, pad bits zero; score.
 */
int acx_ef_crossfusion_debug(acx_ctx *ctx, int32_t i, int32_t j, const acx_ef_params *params, int32_t niters,
                             double reg_diag, float *ssm_a, float *ssm_b, float *csm, double *W, double *D, double *X,
                             uint32_t *bits, float *score);

/*
 * The same chain behind the GEMMs for a caller's three triples of f32 matrices (tests): SA (3, M, M), SB (3, N, N),
 * C (3, M, N).  Also returns r (3, M) and c (3, N), the means of the k2 smallest cells of every row and of the k1
 * smallest of every column of C (getWCSM, similarity_fusion.py:47-51).  M, N <= 1024; the refusals of the call above.
 */
int acx_crossfusion_matrices(acx_ctx *ctx, const float *SA, const float *SB, const float *C, int32_t M, int32_t N,
                             double kappa, int32_t K, int32_t niters, double reg_diag, double *r, double *c, double *W,
                             double *D, double *X, uint32_t *bits, float *score);

/* The selection and the Smith-Waterman alone on a caller's f64 (M, N) matrix (tests).  M, N <= 1024. */
int acx_xsel_binary_sw(acx_ctx *ctx, const double *X, int32_t M, int32_t N, double kappa, uint32_t *bits, float *score);

/* ---- the N x N pair grid -------------------------------------------------- */

/*
 * CoverAlgorithm.all_pairwise (algorithm_template.py:142-192) builds the list of all pairs
 * (itertools.combinations for symmetric algorithms, permutations otherwise, :168-171), cuts it into
 * 45 chunks for joblib (:172-177) and mirrors the result (D += D.T, :189-191).  Here the grid is cut
 * into tile x tile blocks of tracks (upper triangle incl. the diagonal blocks when symmetric),
 * each block costed by the sum of len_i * len_j over its pairs, and the blocks are dealt to `world`
 * ranks longest-processing-time-first.  A rank writes the scores of its blocks into one dense
 * buffer (block after block in deal order; a block is rows x cols x planes floats, planes
 * fastest); the only exchange of the whole path is one all-gather of those buffers.
 */
enum { ACX_ALGO_SERRA09 = 0, ACX_ALGO_CHENFUSION = 1, ACX_ALGO_SIMPLE = 2, ACX_ALGO_EARLYFUSION = 3, ACX_ALGO_FTM2D = 4 };

typedef struct {
    int32_t algo;       /* ACX_ALGO_*: 1 / 2 (qmax, dmax) / 1 / 4 (mfccs, ssms, chromas, early) / 1 score planes */
    int32_t symmetric;  /* 1: unordered pairs i < j   0: ordered pairs i != j (all_pairwise's `symmetric`) */
    int32_t tile;       /* tracks per block edge; 0: 128, halved while a rank would get fewer than 32 blocks */
    int32_t world;      /* number of ranks */
} acx_grid_spec;

typedef struct {
    int32_t row0, col0;   /* first track of the block's rows / columns */
    int32_t rows, cols;   /* tracks per side */
    int32_t rank;         /* owner */
    int32_t diagonal;     /* row0 == col0: only i < j (symmetric) or i != j is computed; the rest stays 0 */
    int64_t offset;       /* float offset of the block in its owner's buffer */
    double cost;          /* sum of len_i * len_j over the block's pairs */
} acx_grid_tile;

typedef struct {
    int32_t sslen;        /* SSLEN (Simple ctor, simple_silva.py:26-27), default 10 */
    int32_t oti;          /* 1: transpose the second track toward the first (Simple.oti) */
} acx_simple_params;

/*
 * The plan: pure host function of (track lengths, spec), identical on every rank.  `tiles` (may be
 * NULL) receives up to `capacity` blocks in deal order (cost descending), *n_tiles their number,
 * floats_per_rank[world] the size of every rank's score buffer, cost_per_rank[world] (may be NULL)
 * the dealt cost.  No device needed.
 */
int acx_grid_plan(const int64_t *lengths, int32_t n_tracks, const acx_grid_spec *spec, acx_grid_tile *tiles,
                  int64_t capacity, int64_t *n_tiles, int64_t *floats_per_rank, double *cost_per_rank);

/* Track lengths the grid of `algo` is planned on: pooled frames (Serra09 / ChenFusion: the f32
 * pool; SiMPle: the f64 pool), blocks (EarlyFusion) or 1 for every track (FTM2D: all pairs cost the
 * same).  lengths: room for `capacity` entries. */
int acx_pool_lengths(acx_ctx *ctx, int32_t algo, int64_t *lengths, int32_t capacity, int32_t *n_tracks);

/*
 * Scores of blocks [first, first + count) of rank `rank`'s deal (count < 0: all of them) into
 * d_scores, a DEVICE buffer of floats_per_rank[rank] floats owned by the caller (e.g. the
 * storage of a torch tensor that is handed to the all-gather next).  The slice's part of the
 * buffer is zeroed first.  params: acx_serra09_params (Serra09, ChenFusion), acx_simple_params,
 * acx_ef_params; FTM2D takes none (NULL; the scores are those of acx_ftm2d_pairs, bit for bit, from a tile
 * kernel that stages both sides' shingles in LDS).  Replaces the similarity(idxs) fan-out of
 * algorithm_template.py:172-187.
 */
int acx_grid_run(acx_ctx *ctx, const acx_grid_spec *spec, const void *params, int32_t rank, int64_t first,
                 int64_t count, float *d_scores);

/*
 * Gathered rank buffers (HOST memory: `world` segments of rank_stride floats) -> the planes of
 * D: D[e][i * ld + j] = score plane e of pair (i, j), for the blocks [first, first + count) of
 * every rank; mirror != 0 also stores D[e][j * ld + i] (the D += D.T of
 * algorithm_template.py:189-191 on a matrix whose other triangle is zero).  Pure host function.
 */
int acx_grid_scatter(const int64_t *lengths, int32_t n_tracks, const acx_grid_spec *spec, const float *gathered,
                     int64_t rank_stride, int64_t first, int64_t count, float *const *D, int64_t ld,
                     int32_t mirror);

/* One GPU, whole grid: plan (world must be 1) + run + scatter into the caller's N x N host planes
 * (e.g. the float32 memmaps CoverAlgorithm.Ds holds). */
int acx_pair_grid(acx_ctx *ctx, const acx_grid_spec *spec, const void *params, float *const *D, int64_t ld,
                  int32_t mirror);

/* ---- ranking of finished score rows: evaluation positions and top-k ----- */

/*
 * Everything a user does with a finished N x N score matrix orders its rows (getEvalStatistics,
 * algorithm_template.py:205-290: the positions of a track's clique mates; candidate lists: the first k columns).
 * Both calls take a ROW SLAB in HOST memory: n_rows rows of n floats with leading dimension ld; row r is the score row
 * of track self[r], whose own cell takes no part.  posn: n distinct non-negative tie ranks, or NULL (= the column index).
 * ONE order: column a comes before column b iff s[a] > s[b], or s[a] == s[b] and posn[a] < posn[b] -- IEEE comparison,
 * so -0.0 and +0.0 tie.
 *   acx_rank_columns  for every listed column m of row r (mates[moff[r] .. moff[r + 1]), any number, moff[0] = 0) its
 *                     1-based position 1 + #{c != self: s[c] > s[m]} + #{c != self: s[c] == s[m], posn[c] < posn[m]}
 *                     into out_pos (moff[n_rows] entries).  A row that holds a NaN or a -inf outside its own cell is
 *                     FLAGGED (out_flag[r] = 1, its positions -1): the host decides what such a row means.  +inf is an
 *                     ordinary value.
 *   acx_topk_rows     the first k columns of the order and their scores (bit copies) into out_idx / out_score
 *                     (n_rows x k).  NaN cells come after every number (after -inf too), among themselves by posn --
 *                     what np.argsort(-row, kind="stable") does.  Fewer than k other columns: the tail is index -1,
 *                     score NaN.  k <= 1024; beyond: ACX_ERR_UNSUPPORTED.
 * The slab goes to the device in pieces of whole rows (64 MB) through two pinned slots, within acx_set_scratch_limit
 * (two rows that do not fit: ACX_ERR_NOMEM); n is not limited by the LDS.  The whole argument list is validated before
 * the first launch (indices in [0, n), moff non-decreasing, a mate equal to self[r] is ACX_ERR_INVALID, the message
 * names the argument); nothing is left in flight on error.
 */
int acx_rank_columns(acx_ctx *ctx, const float *scores, int64_t ld, int32_t n, int32_t n_rows, const int32_t *self,
                     const int32_t *posn, const int64_t *moff, const int32_t *mates, int32_t *out_pos, uint8_t *out_flag);
int acx_topk_rows(acx_ctx *ctx, const float *scores, int64_t ld, int32_t n, int32_t n_rows, const int32_t *self,
                  const int32_t *posn, int32_t k, int32_t *out_idx, float *out_score);

/* ---- queries against the uploaded collection: scores and top-k without N x N */

/*
 * The question a cover-song identification engine is asked: given these Q tracks, which k tracks of the collection are
 * their covers?  Queries and candidates are INDICES into the pool that is already uploaded (the collection and the
 * queries are uploaded together); duplicate queries are allowed.  The queries run in BANDS of up to 128 rows: a band's
 * pairs go through the same pair kernels as acx_*_pairs / acx_grid_run, its scores stay on the device (band rows x
 * n_tracks x planes floats), are normalised and ranked there, and only the results come back.
 *
 *   raw score   of the cell (query q, track c): bit for bit what acx_serra09_pairs / acx_chenfusion_pairs /
 *               acx_simple_pairs (rounded to f32, as Ds['main'] stores it) / acx_earlyfusion_pairs / acx_ftm2d_pairs
 *               return for that pair in the orientation `symmetric` selects.  Planes as in acx_grid_spec.
 *   col_mode    applied once per cell with an IEEE f64 division and ONE rounding to f32 -- the bits of the classes'
 *               normalize_by_length (rqa_serra09.py:71-83: mode 1 with col = sqrt(T_c); latefusion_chen.py:75-85 and the
 *               later `*= -1` of do_late_fusion :90: mode 2)
 *   own column  a query's own column takes no part and is never computed: its cell is 0 in acx_query_scores; acx_query_topk
 *               skips it, also when `cands` lists it
 *   order       the one of acx_topk_rows with posn == NULL: larger score first, -0.0 and +0.0 tie; ties in ascending track
 *               index; -inf is an ordinary value; NaN comes after every number.  Fewer than k candidates: the tail is
 *               index -1, score NaN.  k <= 1024; beyond: ACX_ERR_UNSUPPORTED
 *   memory      a band (its scores plus its results) takes at most HALF of acx_set_scratch_limit, the pair kernels of the
 *               band what is left of a limit the caller set; one row that does not fit: ACX_ERR_NOMEM
 *   errors      the whole argument list is validated before the first launch -- spec (algo, symmetric, col_mode,
 *               reserved == 0), params (NULL only for FTM2D), the pool of spec->algo present (else ACX_ERR_STATE), every
 *               query and candidate a track in [0, n_tracks), `cands` strictly ascending, col present iff col_mode != 0
 *               and finite, k -- and the message names the argument; a failed call leaves nothing in flight
 * params: per algorithm exactly as for acx_grid_run (FTM2D: NULL).
 */
typedef struct {
    int32_t algo;       /* ACX_ALGO_* */
    int32_t symmetric;  /* 1: the pair {q, c} is computed as (min(q, c), max(q, c)), the cell all_pairwise(symmetric=True)
                              computes and mirrors.  0: as (q, c), row q of an ordered grid (SiMPle) */
    int32_t col_mode;   /* 0: s   1: (float)((double)s / col[c])   2: -(float)(col[c] / (double)s)   (s = 0 -> -inf) */
    int32_t reserved;   /* 0 */
} acx_query_spec;

/* The finished rows in full: rows[e][i * ld + c] = plane e of (queries[i], track c); planes of n_queries x ld host floats,
 * ld >= n_tracks.  col: n_tracks values, NULL iff col_mode == 0. */
int acx_query_scores(acx_ctx *ctx, const acx_query_spec *spec, const void *params, const int32_t *queries, int32_t n_queries,
                     const double *col, float *const *rows, int64_t ld);

/* The k first candidates of every query and plane: out_idx / out_score are n_queries x planes x k.  cands: n_cands strictly
 * ascending track indices, or NULL: every track (n_cands is ignored).  Only the candidates' columns are computed. */
int acx_query_topk(acx_ctx *ctx, const acx_query_spec *spec, const void *params, const int32_t *queries, int32_t n_queries,
                   const int32_t *cands, int32_t n_cands, const double *col, int32_t k, int32_t *out_idx, float *out_score);

/* Evaluation of a query set without an N x N matrix: the 1-based positions of listed tracks (a query's clique mates) in
 * the query's finished row -- acx_rank_columns' counting applied to the band's slab on the device.  For every plane e and
 * every listed track m of query i (mates[moff[i] .. moff[i + 1]), any number, moff[0] = 0):
 *     out_pos[e * moff[n_queries] + j] = 1 + #{c != q: s[c] > s[m]} + #{c != q: s[c] == s[m], posn[c] < posn[m]}
 * over EVERY track c of the pool (all columns of the band are computed), s = the finished values of plane e (col_mode as
 * above), IEEE comparisons: -0.0 and +0.0 tie, +inf is an ordinary value.  posn: n_tracks distinct non-negative tie ranks,
 * or NULL (= the track index).  A (query, plane) whose finished values hold a NaN or a -inf outside the query's own column
 * (col_mode 2 turns a raw score of 0 into -inf) is FLAGGED: out_flag[i * planes + e] = 1 and its positions are -1; the
 * host decides what such a row means (acx_query_scores returns it).  Bands and memory as acx_query_topk; every row is
 * charged the longest mate list of the call.  Validated before the first launch, beyond the common rules above: moff[0]
 * == 0 and non-decreasing, every mate a track in [0, n_tracks), a mate equal to its own query is ACX_ERR_INVALID, posn
 * distinct and non-negative; the message names the argument. */
int acx_query_ranks(acx_ctx *ctx, const acx_query_spec *spec, const void *params, const int32_t *queries, int32_t n_queries,
                    const double *col, const int32_t *posn, const int64_t *moff, const int32_t *mates, int32_t *out_pos,
                    uint8_t *out_flag);

/* Reranking: a candidate list PER QUERY -- the second stage of a cascade, whose first stage (a cheap index, acx_query_topk
 * with FTM2D) left every query its own shortlist.  lists: n_queries x list_len int32, row-major; lists[i * list_len + j] is
 * a track in [0, n_tracks) or -1, an empty slot at any position; the entries of a row may be in any order.  A query's own
 * track may be listed and is skipped.  A track listed twice in one row is ACX_ERR_INVALID (the message names the row and
 * both positions); duplicate queries with different lists are fine.
 *   values   raw score, orientation (`symmetric`), col_mode, order, ties, NaN / -inf, k <= 1024 and the -1 / NaN tail are
 *            those of acx_query_topk: row i holds exactly what acx_query_topk(queries = {queries[i]}, cands = the valid
 *            entries of row i, sorted) returns, in indices and score bits
 *   band     rows x list_len x planes floats, laid out by list position -- only the listed cells are computed, a pair two
 *            rows want is computed twice.  Memory per row: 4 list_len planes + 8 planes k bytes within half of
 *            acx_set_scratch_limit (one row that does not fit: ACX_ERR_NOMEM); the rows of a band are bounded by that and
 *            by 2^18 cells, not by 128
 *   errors   the whole argument list is validated before anything is allocated or launched: the common rules above, k,
 *            then the lists (list_len >= 0, lists not NULL when list_len > 0, every entry a track or -1, no track twice
 *            in a row); a failure after that (a listed track shorter than the delay-embedding stack ...) leaves nothing
 *            in flight
 * list_len == 0 or a row of empty slots: all -1 / NaN.  n_queries == 0: ACX_OK. */
int acx_query_topk_lists(acx_ctx *ctx, const acx_query_spec *spec, const void *params, const int32_t *queries, int32_t n_queries,
                         const int32_t *lists, int32_t list_len, const double *col, int32_t k, int32_t *out_idx, float *out_score);

/* Fused scores for query shortlists: similarity network fusion (acx_snf_fuse_dists) is a function of a SET of tracks, so
 * it is defined on a query's neighbourhood -- the query and its shortlist -- as what the classes' late fusion computes on a
 * collection that holds only those tracks.  queries / lists / list_len as in acx_query_topk_lists (any order, -1 = an
 * empty slot, the query's own track is skipped, a track twice in a row is ACX_ERR_INVALID).  For query i:
 *   T        = sorted({queries[i]} U valid entries of row i), ascending track index, n = |T|
 *   scores   every unordered pair of T as the pair (min, max) -- spec->symmetric must be 1 -- with the bits of
 *            acx_chenfusion_pairs / acx_earlyfusion_pairs, mirrored
 *   dists    per fused type t and its planes fused->planes[t][0 .. count[t]) (pair-kernel plane indices, in THIS order: the
 *            sweep's in-place aliasing makes the order matter), an n x n f64 matrix each:
 *              ACX_FUSED_SQRTLEN  (double)(float)(col[c] / (double)s) for column c   (spec->col_mode 2, col = sqrt(T_c):
 *                                 ChenFusion.normalize_by_length's f32 value, widened as do_late_fusion reads it)
 *              ACX_FUSED_INV1P    1 / (1 + (double)s)                                (spec->col_mode 0, col NULL: EarlyFusion)
 *            the diagonal is 0 (the fusion zeroes it whatever it holds)
 *   fusion   acx_snf_fuse_dists(those matrices, K, niters, reg_diag, mu): the SAME bits (the batched kernels run the row
 *            bodies of the single-problem kernels)
 *   ranking  row queries[i] of the fused matrix without its own column, every value rounded ONCE to f32, in the order of
 *            acx_topk_rows (larger first, ties by ascending track index, NaN last, tail -1 / NaN), as collection indices:
 *            out_idx / out_score are n_queries x n_types x k
 *   flag     out_flag[i * n_types + t] = 1 where an off-diagonal distance of type t is not finite (a ChenFusion raw score of
 *            0): that row is NaN as in the whole-collection fusion; the other queries are unaffected
 * With two fused types (EarlyFusion 'late' and 'early+late') the pairs are scored once and fused twice.
 *   cost     n (n - 1) / 2 alignments per query (acx_query_topk_lists: list_len); a pair two neighbourhoods share is
 *            computed twice
 *   memory   the queries of a chunk hold their pair scores, (3 m + 2) n^2 + n doubles (distances, two generations of P,
 *            two work matrices, the local scales), m n K list entries and their results at once, m = the most planes of a
 *            type, within HALF of acx_set_scratch_limit; one neighbourhood that does not fit: ACX_ERR_NOMEM
 *   errors   validated before anything is allocated or launched: the common rules above, spec->symmetric == 1, the struct
 *            (n_types 1..2, count 2..4, planes in [0, planes of the algorithm), transform and its col_mode, reserved == 0,
 *            1 <= K, K > 64: ACX_ERR_UNSUPPORTED, niters >= 1, mu > 0), k, list_len > 1024: ACX_ERR_UNSUPPORTED, the
 *            lists, then n >= K + 2 for every row (the message names the row: the K-neighbour cut of the reference is not
 *            defined below); a failure after that leaves nothing in flight
 * n_queries == 0: ACX_OK. */
#define ACX_FUSED_SQRTLEN 1
#define ACX_FUSED_INV1P 2
typedef struct {
    int32_t n_types;        /* fused types of the call: 1 or 2 */
    int32_t count[2];       /* planes of each type: 2 .. 4 */
    int32_t planes[2][4];   /* their pair-kernel plane indices, in fusion order */
    int32_t transform;      /* ACX_FUSED_* */
    int32_t K, niters;      /* do_late_fusion: 20, 20 */
    int32_t reserved;       /* 0 */
    double reg_diag, mu;    /* do_late_fusion: 1, 0.5 */
} acx_fused_spec;

int acx_query_fused_lists(acx_ctx *ctx, const acx_query_spec *spec, const void *params, const int32_t *queries, int32_t n_queries,
                          const int32_t *lists, int32_t list_len, const double *col, const acx_fused_spec *fused, int32_t k,
                          int32_t *out_idx, float *out_score, uint8_t *out_flag);

/* ---- appends: tracks behind an uploaded pool, and away again ------------- */

/*
 * The query calls above take their queries from the uploaded pool.  A track the collection does not hold is put BEHIND the
 * pool -- O(new tracks) work, the collection stays where it is --, asked about as queries n_old .. n_old + n_new - 1 against
 * the candidates [0, n_old), and taken away again with acx_pool_truncate.
 *
 * The rule: after an upload and ANY sequence of appends and truncates, every later call (pairs, debug entry points,
 * acx_pool_lengths, acx_download_pool*, the pair grid, the query calls) returns the bits it returns after ONE upload of the
 * same final track list, for every parameter set.  Data derived from the pool (the active copy for tau > 1, the rotated and
 * f16 operand pools, the norm table, window norms, row norms, row scales and splits) is extended for the new tracks only.
 *
 * Arguments are those of the upload call of the same pool; `offsets` (n_new + 1 entries) are relative to the appended
 * tracks, offsets[0] == 0.  A pool block that is too small is replaced by one of max(need, 1.5 x its capacity) and keeps the
 * capacity afterwards, so append -> query -> truncate in a loop allocates nothing after the first round.  Errors, all found
 * before the pool is changed -- unlike an upload, a failed append leaves the pool exactly as it was: no pool of that kind, or
 * an EarlyFusion / FTM2D pool still open: ACX_ERR_STATE; n_new < 1, offsets that do not start at 0 or decrease, dim / dims
 * other than the pool's, more than 2^31 - 1 tracks in all: ACX_ERR_INVALID naming the argument; a failed allocation:
 * ACX_ERR_NOMEM; a non-finite value: as in the upload (acx_set_nonfinite_policy), the track named by its index in the pool
 * AFTER the append; acx_nonfinite_zeroed counts the values the last upload OR append zeroed.
 *   acx_pool_append            pooled f32 frames behind the pool of acx_upload_pool / acx_upload_raw_pool
 *   acx_pool_append_raw        raw chroma: block medians of `fac` frames written straight behind the pool's end, the OTI's
 *                              chroma profile summed on the device (same bits as the upload's host loop); pooled_offsets_out
 *                              (n_new + 1 entries, may be NULL) receives the new tracks' relative pooled offsets
 *   acx_pool_append_f64        SiMPle features behind the pool of acx_upload_pool_f64
 *   acx_ef_pool_append         block features of n_new tracks behind a finished EarlyFusion pool.  The call takes no dims: rows
 *                              have the widths the pool was begun / uploaded with, and offsets[n_new] rows of exactly those
 *                              widths are read from each array.  THE WIDTHS ARE THE CALLER'S RESPONSIBILITY: the library
 *                              cannot check them, and narrower rows make it read past the end of the host arrays
 *   acx_ftm2d_append_shingles  (n_new, dim) f64 shingles behind a finished FTM2D pool; dim = the pool's
 *   acx_pool_truncate          keep the first n_tracks tracks of the pool of `algo` (ACX_ALGO_*; Serra09 and ChenFusion share
 *                              one), 1 <= n_tracks <= the current count (equal: nothing happens); the capacity is kept
 */
int acx_pool_append(acx_ctx *ctx, const float *frames, const int64_t *offsets, int32_t n_new, int32_t dim);
int acx_pool_append_raw(acx_ctx *ctx, const float *raw, const int64_t *raw_offsets, int32_t n_new, int32_t dim, int32_t fac,
                        int64_t *pooled_offsets_out);
int acx_pool_append_f64(acx_ctx *ctx, const double *frames, const int64_t *offsets, int32_t n_new, int32_t dim);
int acx_ef_pool_append(acx_ctx *ctx, const float *mfccs, const float *ssms, const float *chromas, const double *chroma_med,
                       const int64_t *offsets, int32_t n_new);
int acx_ftm2d_append_shingles(acx_ctx *ctx, const double *shingles, int32_t n_new, int32_t dim);
int acx_pool_truncate(acx_ctx *ctx, int32_t algo, int32_t n_tracks);

/* ---- multi-GPU inside the library: RCCL over xGMI, no Python ------------- */

/*
 * The reference fans its pair list out over joblib processes (algorithm_template.py:172-177); the Python host of this
 * library runs one process per GPU under torch.distributed (acoss_amd/dist.py).  A host WITHOUT Python gets the same path
 * from the library itself: one context (one GPU) per process or thread, one RCCL communicator rank per context.  librccl
 * is dlopen()ed on first use (env ACX_RCCL_LIB, a copy the process already holds, the one next to the HIP runtime, the
 * system's): single-GPU users never load it.
 *   acx_comm_id         rank 0: a fresh communicator id (ACX_COMM_ID_BYTES = sizeof(ncclUniqueId)); the HOST carries
 *                       it to the other ranks by whatever means it has (MPI, a socket, a file)
 *   acx_comm_init       every rank: join (collective: returns when all `world` ranks have called it)
 *   acx_grid_allgather  the one exchange of the path: every rank's score buffer (floats_per_rank floats at d_local,
 *                       what acx_grid_run filled) into d_gathered (world x floats_per_rank floats, DEVICE memory, rank r
 *                       at r * floats_per_rank) -- ncclAllGather on the library's stream, behind the kernels, device
 *                       to device over xGMI; returns when the buffer is complete
 *   acx_pair_grid_ranks the whole grid: plan, this rank's tiles, the all-gather, rank 0 scatters into its planes
 *                       (spec->world is ignored: the communicator's size is used; D may be NULL on ranks > 0).
 *                       A collective: every rank calls it with the same spec and params after uploading the same pool.
 *   acx_comm_destroy    leave (also done by acx_destroy)
 */
#define ACX_COMM_ID_BYTES 128
int acx_comm_id(void *id_out);
int acx_comm_init(acx_ctx *ctx, const void *id, int32_t rank, int32_t world);
int acx_comm_destroy(acx_ctx *ctx);
int acx_grid_allgather(acx_ctx *ctx, const float *d_local, float *d_gathered, int64_t floats_per_rank);
int acx_pair_grid_ranks(acx_ctx *ctx, const acx_grid_spec *spec, const void *params, float *const *D, int64_t ld,
                        int32_t mirror);

/* ---- device buffers for hosts without a GPU runtime of their own -------- */

/* acx_grid_run / acx_grid_allgather work on DEVICE buffers the caller owns.  A Python host takes them from torch; a host
 * that links no GPU runtime (and bench.py at one GPU, which then never imports torch) takes them from here: zero-filled
 * hipMalloc on the context's device; acx_dev_read drains the library's stream and copies to the host; acx_dev_sync =
 * hipDeviceSynchronize.  Buffers still alive are freed with the context. */
int acx_dev_alloc(acx_ctx *ctx, int64_t bytes, void **d_ptr);
int acx_dev_free(acx_ctx *ctx, void *d_ptr);
int acx_dev_read(acx_ctx *ctx, void *host_dst, const void *d_src, int64_t bytes);
int acx_dev_sync(acx_ctx *ctx);

/* ---- measurement -------------------------------------------------------- */

/* Per-kernel timing with HIP events recorded on the library's own stream around
 * every launch (bench.py's roofline leg).  Off by default.  While it is on, every
 * kernel runs on that one stream: the Serra09 alignment sweeps, which otherwise run
 * on a second stream beside the next band kernels, are timed alone, not beside
 * another launch -- a call is a few percent slower with the clocks on than without. */
int acx_profile_enable(acx_ctx *ctx, int on);
int acx_profile_reset(acx_ctx *ctx);
int acx_profile_count(const acx_ctx *ctx);
/* kernel `idx`: name (NUL-terminated into name[name_len]), accumulated
 * milliseconds, launches, and the number of pair-cells (Mq*Mr summed) it covered. */
int acx_profile_get(acx_ctx *ctx, int idx, char *name, int name_len,
                    double *ms, int64_t *launches, int64_t *cells);

/* device-side sqrt probe used by the parity tests (must be correctly rounded) */
int acx_debug_sqrt(acx_ctx *ctx, const float *in, int64_t n, float *out);
/* the sqrt of the EarlyFusion distance epilogues (v_sqrt_f32 + one Newton step: within 1 ulp, almost always exact) */
int acx_debug_ef_sqrt(acx_ctx *ctx, const float *in, int64_t n, float *out);

/* ---- debug: history independence ---------------------------------------- */

/* No result may depend on what device memory held before a call.  These two exports let a test decide what that is (tests/
 * test_gpu_arena_history.py); they use no environment variable and change nothing while unused.
 *
 * acx_debug_set_alloc_fill   process-wide.  While `on`, every DEVICE block the library allocates (the contexts' grow-only arenas and
 *                            pools, and the work buffers an entry point allocates for the length of a call) is filled with `word`
 *                            before anyone uses it.  Pinned host buffers are not filled; acx_dev_alloc stays zero-filled.
 * acx_debug_fill_arenas      drains the context's streams, fills TO CAPACITY every device block of the context that is scratch --
 *                            sized per call, no input: DESIGN.md lists every block of a context with its class -- and waits.
 *                            Uploaded and derived pools, and the descriptor blocks the host uploads before every launch, keep
 *                            their contents. */
int acx_debug_set_alloc_fill(int on, uint32_t word);
int acx_debug_fill_arenas(acx_ctx *ctx, uint32_t word);

#ifdef __cplusplus
}
#endif
#endif /* ACX_H */
