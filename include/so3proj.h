/* so3proj.h -- C ABI of libso3proj.so: batched 3x3 SVD -> SO(3) projection on AMD MI355X (gfx950).
 *
 * Drop-in boundary for the hot path of henrikgruner/PoseEstimation.  The reference has no FFI (it is
 * pure Python bottoming out in ATen); each entry point below replaces one ATen op chain of the
 * reference, cited as <file>:<lines> relative to the reference repository root.  A Python binding
 * with the reference's own function names lives in poseestimation_amd/rotation_representation.py;
 * the ctypes stub a maintainer would add to the reference is shown in INTEGRATION.md.
 *
 * Conventions (all entry points)
 *   - Plain pointers and sizes only; no torch / HIP C++ types.  `stream` is a hipStream_t passed as
 *     void* (NULL = the legacy default stream).
 *   - All pointers are DEVICE pointers owned by the caller.  The library never allocates or frees
 *     device memory and keeps no pointer after the call returns.
 *   - Enqueue-only: every call launches on `stream` and returns without synchronising; no hidden
 *     hipMalloc / hipMemcpy / hipDeviceSynchronize, so calls are hipGraph-capturable.  The caller
 *     selects the device (hipSetDevice) -- the library holds no global mutable state and is
 *     re-entrant from several host threads and devices.
 *   - Layout: row-major contiguous 3x3 blocks; (B,9) == (B,3,3); element (i,j) of matrix b at
 *     offset 9*b + 3*i + j.  16-byte aligned base pointers take the vectorised path, any 4-byte
 *     (2-byte for bf16) aligned pointer is accepted.
 *   - Return value: 0 on success, otherwise a hipError_t value (or SO3_ERR_INVALID for a bad
 *     argument); so3_last_error() gives a thread-local description.  Nothing throws.
 *   - NaN/Inf in -> NaN out (the reference's CPU path raises from LAPACK instead; the reference's GPU
 *     path returns NaN; documented divergence).
 *   - B == 0 is a no-op that returns 0.
 */
#ifndef SO3PROJ_H_
#define SO3PROJ_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SO3PROJ_VERSION 210          /* 0.2.0: the reducing entry points exist once (*_v2: workspace nullable, a flags word), the float64 ones
                                        included (so3_angle_error_v2_f64, so3_frob_loss_v2_f64: round 4 had changed their arguments under the old
                                        names); so3_angle_stats's workspace is zero-filled once by the caller.  0.2.1 (210) ADDS the metrics'
                                        backward (so3_angle_bwd_f32 / _f64), so3_geodesic_eps_f64, two flags and the cloud backwards
                                        (so3_kabsch_bwd_f32, so3_rotate_clouds_bwd_f32); nothing of 200 changed its
                                        arguments, but the float64 entries now reject flag bits they do not know.  A binding checks so3_version(). */
#define SO3_ERR_INVALID (-1)

/* Library version (SO3PROJ_VERSION the library was built with).  A caller compiled against another version of this header must not
 * call the library: argument lists changed between 100 and 200 without new symbol names for every function (210 only adds to 200). */
int so3_version(void);

/* Thread-local description of the last non-zero return on this thread ("" if none). */
const char *so3_last_error(void);

/* Name of the streaming-engine kernel this thread launched last, as a profiler prints it
 * ("so3::k_rows<so3::OpProject<4, false, 100, true>, 2, 3, 256, false, false, 1>"; "" if none yet): the runtime's name
 * of the kernel behind the launch, demangled, so a bench line or a log names the instantiation that actually ran. */
const char *so3_last_kernel(void);

/* ---- K1: symmetric orthogonalization -------------------------------------------------------------
 * R_b = U diag(1,1,det(U V^T)) V^T for M_b = U S V^T.
 * Replaces rotation_representation.py:192-206 (view -> torch.svd -> transpose -> matmul -> det ->
 * cat -> matmul; copies at 3D-Pose/main2.py:34-48, point_cloud/model_fetch.py:13-27, ...).
 *   M    in   B*9 elements (f32, or bf16 bits for the _bf16 variant)
 *   R    out  B*9 float32 (always float32: a bf16 rotation is not orthogonal to 1e-5)
 *   flip out  optional (NULL to skip), B bytes: 1 where det(U V^T) < 0 (<=> det M < 0), else 0
 */
int so3_project_fwd_f32(const float *M, float *R, uint8_t *flip, int64_t B, void *stream);
int so3_project_fwd_bf16(const void *M, float *R, uint8_t *flip, int64_t B, void *stream);

/* K1 over n independent buffer pairs in ONE launch of the streaming engine: R[i] = the rotations of M[i], B[i] rows each.
 *   1 <= n <= 8; every B[i] a positive multiple of 64; every M[i], R[i] non-NULL and 4-byte aligned; the rounds of all segments
 *   together fit 32 bits (2^31 - 4096 units of 64 rows).  Anything else returns SO3_ERR_INVALID and launches nothing.
 *   The three arrays are host memory and are read before the call returns.  The segments run concurrently inside the kernel: no
 *   R[i] may overlap another R[j] or any M[j] (the caller's contract, as for separate launches on separate streams).
 * Every row goes through the arithmetic of so3_project_fwd_f32, paired with the same neighbour row: the results are bit-identical
 * to n separate calls; with n = 1 it IS that call's launch.  What it saves is the launch boundary: the tail of one segment overlaps
 * the fill of the next inside the kernel. */
int so3_project_fwd_segments_f32(const float *const *M, float *const *R, const int64_t *B, int n, void *stream);

/* Capture-time fusion of adjacent K1 calls.  While a stream is being CAPTURED into a graph, a call of so3_project_fwd_f32 / _bf16
 * with flip == NULL, B a multiple of 64 and 4-byte aligned pointers may add no kernel node of its own: it is folded, as one more
 * segment, into the node that the SAME thread's previous such call created, when that node is the stream's only capture
 * dependency (nothing was captured on the stream in between, and nothing else must precede the call), both calls are the same
 * instantiation, the node holds fewer than 8 segments, and the new call's buffers are hazard-free against the node's (input
 * overlaps no earlier output; output overlaps no earlier output or input).  Results are the same bits; a replay runs one persistent
 * launch per run of up to 8 calls and a profiler sees one dispatch for it.  Eager (uncaptured) calls are never fused.
 *   so3_capture_fusion(enable)      sets the process-wide switch (default: on) and returns the previous setting.  A caller that
 *                                   edits the kernel-node parameters of a captured graph itself switches it off before capturing.
 *   so3_capture_fused_launches()    how many calls THIS thread has folded into an earlier node so far. */
int so3_capture_fusion(int enable);
int64_t so3_capture_fused_launches(void);
/* The fusion decision alone, for tests (no device, no pointer is dereferenced): would a call (M, R, B rows, elem_bytes = 4 for
 * float32 / 2 for bfloat16 input) be folded into a recorded node of rec_n segments (rec_M, rec_R, rec_B, rec_elem_bytes), given
 * whether the capture is the same, how many capture dependencies the stream has and whether the first is the recorded node?
 * Returns 1 / 0, or SO3_ERR_INVALID for a malformed record. */
int so3_capture_fusion_would_fuse(const void *const *rec_M, void *const *rec_R, const int64_t *rec_B, int rec_n, int rec_elem_bytes,
                                  int same_capture, int ndeps, int dep_is_recorded_node, int elem_bytes, const void *M, const void *R,
                                  int64_t B);

/* ---- K2: backward of K1 ---------------------------------------------------------------------------
 * dM_b = U' Bm V^T with the signed SVD M = U' diag(s') V^T (U', V in SO(3)), A = U'^T G V,
 * Bm_ij = (A_ij - A_ji)/(s'_i + s'_j), Bm_ii = 0.  The SVD is recomputed from M (nothing else is
 * saved by the forward).  Replaces autograd's svd_backward + the backward of the glue ops triggered
 * at 3D-Pose/main.py:90, UPNA/main.py:63, Comparison/main.py:62.
 * Denominators are clamped at 1e-12*s1 (the reference yields inf/NaN at s'_i + s'_j = 0).
 *   M  in  B*9 (f32 / bf16),  G in B*9 float32 (dL/dR),  dM out B*9 (f32 / bf16)
 */
int so3_project_bwd_f32(const float *M, const float *G, float *dM, int64_t B, void *stream);
int so3_project_bwd_bf16(const void *M, const float *G, void *dM, int64_t B, void *stream);

/* float64 variants (the reference's functions accept double tensors; callers on the hot path never pass them):
 * M, R, G, dM are B*9 float64.  Same algorithm in float64 arithmetic, sweeps repeated until the residual is below
 * 1e-14; one row per thread, not tuned.  flip (nullable) as above. */
int so3_project_fwd_f64(const double *M, double *R, uint8_t *flip, int64_t B, void *stream);
int so3_project_bwd_f64(const double *M, const double *G, double *dM, int64_t B, void *stream);

/* ---- the reducing entry points: K3, K3', K4, K1+K4 ----------------------------------------------------------------
 * Each reduces over the batch (loss_sum; sum_count, range_flag) and exists ONCE; how the reduction is finished is chosen by
 * `workspace` and `flags`:
 *   workspace  NULL, or so3_reduce_workspace_bytes() bytes of device memory owned by the caller, ZERO-FILLED ONCE before its
 *              first use (every call leaves it zeroed), used by ONE stream at a time.  With it every workgroup parks its
 *              partial in a slot of its own and the last one to finish (a ticket) sums the slots in a fixed order and writes
 *              the results with plain stores: one launch, and the same input gives the same bits whatever order the
 *              workgroups retire in.  Without it the accumulators are zeroed by a memset / 1-thread launch in front of the
 *              kernel (unless SO3_PREZEROED) and every workgroup adds to them with one atomic.  (Batches of <= 1024 rows run
 *              as one workgroup and never touch it; input that cannot take the streaming engine -- e.g. a bfloat16 view
 *              starting at an odd row -- falls back to the atomics path.)
 *   flags      SO3_RADIANS    angles in radians (default: degrees)                                        [K4, K1+K4]
 *              SO3_PREZEROED  the caller guarantees loss_sum[0] / sum_count[0] / *range_flag are 0 on entry (e.g. fresh slots
 *                             of a zero-filled pool): no init launch, the kernels add to them as they are and one workgroup
 *                             stores the row count into sum_count[1]
 *              SO3_EXACT_F64  K1+K4's sum without per-row angles: the reference's float64 arithmetic on EVERY row (default:
 *                             float32 trace and acos for rows whose cosine is at least 5e-7 away from +-1, float64 inside
 *                             that band; see so3_project_angle_error_v2_f32)
 */
#define SO3_RADIANS 0x1u
#define SO3_PREZEROED 0x2u
#define SO3_EXACT_F64 0x4u
#define SO3_GRAD_SCALAR 0x8u         /* so3_angle_bwd_*: `grad` is ONE element in device memory shared by every row */
#define SO3_F64_MATH 0x10u           /* so3_angle_bwd_f32: angle_error's spelling (float64 arithmetic on float32 data, float64 `grad`) */
size_t so3_reduce_workspace_bytes(void);

/* ---- K3: fused head forward + Frobenius loss + backward (config #4) ------------------------------
 * loss = mean_b ||Rtrue_b - R_b||_F  (3D-Pose/loss.py:7-11; NOT squared),  dM = dloss/dM.
 * Replaces the chain 3D-Pose/main.py:60 (head), :85 (loss), :90 (backward) in one launch.
 *   M         in   B*9 (f32 / bf16)
 *   Rtrue     in   B*9 float32
 *   R         out  optional B*9 float32
 *   dM        out  optional B*9 (f32 / bf16): d(mean loss)/dM, i.e. already divided by B
 *   loss_sum  out  1 double: sum_b ||Rtrue_b - R_b||_F (may be NULL for B <= 1024 when loss_mean is given)
 *   loss_mean out  optional 1 float: (float)(loss_sum / B) -- what loss_frobenius returns (3D-Pose/loss.py:11), so the host
 *                  side needs no launch of its own to turn the float64 sum into the float32 mean
 * A row whose difference is exactly zero contributes zero gradient (the reference gives NaN).
 */
int so3_frob_fwd_bwd_v2_f32(const float *M, const float *Rtrue, float *R, float *dM, double *loss_sum, float *loss_mean,
                            void *workspace, unsigned flags, int64_t B, void *stream);
int so3_frob_fwd_bwd_v2_bf16(const void *M, const float *Rtrue, float *R, void *dM, double *loss_sum, float *loss_mean,
                             void *workspace, unsigned flags, int64_t B, void *stream);

/* K3': stand-alone Frobenius loss for a caller that already holds R_pred (3D-Pose/loss.py:7-11; copies at
 * Comparison/main.py:12-16, UPNA/main.py:27-31, Iterative/loss.py:4-7):
 *   loss_sum out 1 double: sum_b ||Rtrue_b - Rpred_b||_F;  loss_mean out optional 1 float, as above
 *   dRpred   out optional B*9 float32: d(mean loss)/dRpred = (Rpred - Rtrue)/(B ||.||_F); d/dRtrue is its negative.
 */
int so3_frob_loss_v2_f32(const float *Rpred, const float *Rtrue, float *dRpred, double *loss_sum, float *loss_mean,
                         void *workspace, unsigned flags, int64_t B, void *stream);

/* ---- K4: geodesic angle error ----------------------------------------------------------------------
 * theta_b = acos(clamp((tr(R1_b^T R2_b) - 1)/2, -1, 1)) evaluated in float64 on float32 data.
 * Replaces rotation_representation.py:230-242 (angle_error; copies at Comparison/main.py:19-31,
 * Iterative/utility.py:35-47, ...).
 *   deg        out optional B doubles: angle in degrees (radians with SO3_RADIANS)
 *   sum_count  out optional 2 doubles: (sum_b theta_b, B), accumulated on the device.  This pair is what one RCCL
 *                  all-reduce sums across GPUs.
 *   range_flag out optional 1 int32: set to 1 if any cos is outside [-1.1, 1.1] -- the condition
 *                  on which the reference raises ValueError (:237-239); 0 otherwise.
 */
int so3_angle_error_v2(const float *R1, const float *R2, double *deg, double *sum_count, int32_t *range_flag,
                       void *workspace, unsigned flags, int64_t B, void *stream);

/* K1 + K4 fused: theta_b = angle(proj(M_b), Rtrue_b), R not materialised unless requested -- the evaluation step
 * `angle_error(func[rot_rep](out), R).mean()` of 3D-Pose/main.py:60-62,110-112 and UPNA/main.py:54-57 in one
 * launch reading 72 B per row.  deg / sum_count / range_flag as in so3_angle_error_v2; R optional (required only when B is
 * not a multiple of 64 or a pointer is not 16-byte aligned: the tail then runs as K1 followed by K4 and needs the buffer).
 * Arithmetic of the metric: with `deg` every row's angle is the reference's float64 expression on the float32 rotation
 * (1e-9 degrees against so3_angle_error_v2 on the materialised R).  The SUM ALONE (deg == NULL, batches above 1024 rows on the
 * streaming engine) evaluates the same expression in float32 -- trace, cosine, acos -- for every row whose cosine is at least
 * 5e-7 away from +-1, accumulates in float64, and runs the float64 expression for the rows inside that band (angles within
 * 0.057 degrees of 0 or 180, where acos would amplify the float32 trace's round-off): a row then differs from its float64 angle
 * by at most 2e-7 / sin(theta) rad, without bias; measured |difference of the means| 3e-8 degrees over 1M and 16M Haar pairs and
 * <= 2e-6 degrees when every angle is 0.3 degrees (tests/test_gpu_parity.py).  SO3_EXACT_F64 selects float64 for every row. */
int so3_project_angle_error_v2_f32(const float *M, const float *Rtrue, float *R, double *deg, double *sum_count,
                                   int32_t *range_flag, void *workspace, unsigned flags, int64_t B, void *stream);

/* ---- K4s / K3s: the metric and the loss up to a symmetry group (added in 210) ------------------------------------
 * For objects whose shape a rotation leaves unchanged (ModelNet10-SO(3)'s bathtub, table: 3D-Pose/test_per_class.py:188) the
 * ground truth is defined up to the group.  The group acts on the PREDICTION from the right, as 3D-Pose/loss.py:14-24
 * (rotate_by_180: R_guess @ Rx(pi), ...): a row's candidates are Rpred_b S_k.
 *   S          in   num_classes*K*9 float32: class c's rotations S_{c,0} = I, S_{c,1}, ..., S_{c,K-1} (a class with fewer elements
 *                   padded with the identity).  Orthogonality is the caller's to check (the Python layer does, in float64).
 *   class_id   in   B int32 class of each row: required when num_classes > 1, NULL for one class.  An id outside [0, num_classes)
 *                   gives the row NaN (angle, loss) and index -1.
 *   index      out  optional B int32: the smallest k attaining the row's minimum (k* = 0 wherever the identity is among the best)
 * Limits: 1 <= K <= 64, num_classes >= 1, num_classes * K <= 256; B = 0 is a no-op.
 * so3_sym_angle_error_f32: deg_b = min_k angle(Rpred_b S_k, Rtrue_b), float64 degrees (radians with SO3_RADIANS) on float32 data.
 *   k = 0 is so3_angle_error_v2's arithmetic bit for bit; a further candidate's trace is sum_lj S_lj M_lj in float64 with
 *   M = Rpred^T Rtrue.  With the table {I} the result equals so3_angle_error_v2's.
 *   flags_out  out optional 1 int32, zeroed by the call: bit 0 = some identity cosine outside [-1.1, 1.1] (the reference's raise),
 *                  bit 1 = some class id out of range.
 * so3_sym_frob_loss_f32: loss = mean_b min_k ||Rtrue_b - Rpred_b S_k||_F (not squared) and the gradient of the selected branch
 *   at unit upstream scale: dRpred = -(Rtrue - Rpred S_k*) S_k*^T / (B d), dRtrue = (Rtrue - Rpred S_k*) / (B d), 0 at d = 0.
 *   The selection compares float32 traces of M; the winner's distance and gradient come from Rtrue - Rpred S_k* directly.  With
 *   the table {I} it is so3_frob_loss_v2_f32.
 *   dRpred, dRtrue  out optional B*9 float32;  loss_sum out 1 double;  loss_mean out optional 1 float;
 *   workspace  as so3_frob_loss_v2_f32 (used above 1024 rows; NULL: a memset and atomics instead).  flags: none defined (0).
 */
int so3_sym_angle_error_f32(const float *Rpred, const float *Rtrue, const float *S, const int32_t *class_id, int32_t num_classes,
                            int32_t K, double *deg, int32_t *index, int32_t *flags_out, unsigned flags, int64_t B, void *stream);
int so3_sym_frob_loss_f32(const float *Rpred, const float *Rtrue, const float *S, const int32_t *class_id, int32_t num_classes,
                          int32_t K, float *dRpred, float *dRtrue, int32_t *index, double *loss_sum, float *loss_mean,
                          void *workspace, unsigned flags, int64_t B, void *stream);

/* ---- ADD, ADD-L1 and MSSD up to a symmetry group ---------------------------------------------------------------------
 * The point-based scores of a full pose (so3_add_l2_f32, so3_add_l1_f32) minimised over a discrete symmetry group: the training
 * loss min_k ADD(T_gt, T_pred S_k) and, with a maximum over the points, BOP's MSSD (maximum symmetry-aware surface distance).
 * O(N K) per sample.  S, class_id, num_classes, K: the table of so3_sym_angle_error_f32, same layout and limits; the group acts on
 * the PREDICTION from the right and only rotations about the model origin are supported (no translation part; MSPD, which needs
 * camera intrinsics, is out of scope).  Tgt, Tpred, points as so3_add_l1_f32.
 * The arithmetic is part of the definition (poseestimation_amd/csrc/so3_device.h, sym_add_*):
 *   A_k = Rpred S_k, one float32 fmaf chain per entry in a fixed order; A_0 = Rpred itself, no product
 *   D_k = Rgt - A_k,  dt = tgt - tpred,  d_i^k = D_k p_i + dt in so3_add_l1_f32's fmaf order; a distance comes from these coordinate
 *   differences only, so Tpred S_j == Tgt in float32 makes candidate j exactly 0.
 *   flags (the mode)        statistic of candidate k                        gradient
 *   SO3_SYM_ADD_L2          (1/N) sum_i |d_i^k|_2                           u = d / |d|, 0 at d = 0;  c = grad_scale / N
 *   SO3_SYM_ADD_L1          (1/3N) sum_i (|d_x| + |d_y| + |d_z|)            u = sgn(d), sgn(0) = 0;   c = grad_scale / (3N)
 *   SO3_SYM_ADD_MAX         max_i |d_i^k|_2 (one sqrt, after the maximum)    none: evaluation only (MSSD)
 *   dists[b] = min_k stat_k;  index[b] = the smallest k attaining it (strict < in ascending k: a NaN candidate never wins, a NaN
 *   candidate 0 is never beaten).  The gradient is the selected branch's, w.r.t. Tpred only: with G = sum_i u_i p_i^T and
 *   g_t = sum_i u_i,  dRpred = -c G S_k*^T  (k* = 0: -c G),  dtpred = -c g_t,  bottom row 0.
 *   dists      out optional B float32;  index out optional B int32
 *   loss_sum   out optional double[1] = sum_b dists[b], WRITTEN (not added to), summed in a fixed order without atomics: two calls
 *                  give the same bits.  With dists it is a second small launch over them; without dists ONE workgroup runs the
 *                  whole call (correct, and slow for a large batch: pass dists).
 *   dTpred     out optional B*16 float32 at scale grad_scale; must be NULL with SO3_SYM_ADD_MAX (SO3_ERR_INVALID otherwise)
 * A class id outside [0, num_classes): dists[b] = NaN, index[b] = -1, loss_sum NaN, and the row's twelve gradient entries NaN (as
 * so3_sym_frob_loss_f32 leaves its row), the bottom row still 0; other rows are untouched by it.
 * Limits: 0 <= B <= 2^31, 1 <= N <= 150 000 000 (so3_add_l1_f32's: a cloud's 12 N bytes are addressed in 32 bits), the table's
 * limits above; B = 0 is a no-op.  A sum runs in sweeps of 1024 points -- per lane in index order, the wave's butterfly, the sweeps'
 * totals in order -- so a row's bits depend on its data and N only, never on B or the launch shape.
 */
#define SO3_SYM_ADD_L2 0u
#define SO3_SYM_ADD_L1 1u
#define SO3_SYM_ADD_MAX 2u
int so3_sym_add_f32(const float *Tgt, const float *Tpred, const float *points, const float *S, const int32_t *class_id,
                    int32_t num_classes, int32_t K, float *dists, int32_t *index, double *loss_sum, float *dTpred,
                    float grad_scale, unsigned flags, int64_t B, int32_t N, void *stream);

/* Diagnostic: K1 one row per thread (the same arithmetic, bit for bit, as so3_project_fwd_f32) plus, per row, the device's own
 * verdict: hard[b] = 1 where the quaternion fast path did not certify its result and the row was redone by the Jacobi path.
 * For tests that search for inputs the certificate wrongly accepts (tests/test_gpu_parity.py); not a production entry point. */
int so3_project_fwd_diag_f32(const float *M, float *R, uint8_t *hard, int64_t B, void *stream);

/* dst[i] = src[i] * (*factor), factor a float32 scalar IN DEVICE MEMORY, n elements (float32 / bfloat16; dst may be src).
 * The last step of the chain rule for K3's stored gradient: `loss.backward()` hands the upstream factor over as a 0-dim device
 * tensor, and scaling by it is one launch here instead of a float() / mul / to(bfloat16) chain of the host framework. */
int so3_scale_f32(const float *src, const float *factor, float *dst, int64_t n, void *stream);
int so3_scale_bf16(const void *src, const float *factor, void *dst, int64_t n, void *stream);

/* float64 arguments (the reference's metric and loss functions accept double tensors; rotation_representation.py:232-233 even
 * casts to double itself): the same quantities from float64 data in float64 arithmetic, one row per thread and trip.
 * so3_geodesic_f64 returns float64 radians, so3_frob_loss_v2_f64's dRpred and loss_mean are float64 (loss_mean = loss_sum / B),
 * everything else as in the float32 functions.  `workspace` (nullable) as for the float32 reductions: with it -- and for any batch
 * of <= 1024 rows -- a call is ONE launch whose last workgroup writes sum, count, flag / loss and mean; without it the
 * accumulators are zeroed by a launch in front of the kernel (and the mean written by one behind it).  flags: SO3_RADIANS. */
int so3_angle_error_v2_f64(const double *R1, const double *R2, double *deg, double *sum_count, int32_t *range_flag, void *workspace,
                           unsigned flags, int64_t B, void *stream);
int so3_geodesic_f64(const double *R1, const double *R2, double *theta, int64_t B, void *stream);
int so3_frob_loss_v2_f64(const double *Rpred, const double *Rtrue, double *dRpred, double *loss_sum, double *loss_mean, void *workspace,
                         unsigned flags, int64_t B, void *stream);

/* Float32 radians variant: tr(m1 m2^T), hard clamp to [-1,1], no range check.
 * Replaces rotation_representation.py:209-227 (compute_geodesic_distance_from_two_matrices; copy at
 * point_cloud/main.py:43-57). */
int so3_geodesic_f32(const float *R1, const float *R2, float *theta, int64_t B, void *stream);

/* The same angle with the clamp drawn in by eps and reduced over the batch: geodesic(R1, R2, reduction) of
 * point_cloud/main.py:61-73 (eps = 1e-7: acos(clamp((tr(R1 R2^T) - 1)/2, -1 + eps, 1 - eps)), float32; never called by the
 * reference's loops, kept beside compute_geodesic_distance_from_two_matrices there).
 *   theta  out optional B floats (reduction "none")
 *   sum    optional 1 double of scratch: zeroed by the call, receives sum_b theta_b (float64 accumulation)
 *   result out optional 1 float (needs `sum`): (float) of that sum, or of sum / B when mean != 0 -- written on `stream` behind the kernels
 *   workspace optional so3_reduce_workspace_bytes() of device memory (zeroed once, private to the stream): the reduction is
 *          finished by the kernel's last workgroup -- one launch instead of memset + kernel + mean, and a sum that does not
 *          depend on the order the workgroups finish in
 */
int so3_geodesic_eps_f32(const float *R1, const float *R2, float *theta, double *sum, float *result, int mean, float eps,
                         void *workspace, int64_t B, void *stream);

/* float64 twin of so3_geodesic_eps_f32 (the reference's geodesic() computes in its arguments' dtype): theta B doubles (nullable),
 * sum 1 double of scratch (nullable; zeroed by the call), result 1 double (nullable, needs sum): sum or sum / B.  One row per thread,
 * memset + kernel (+ a 1-thread launch for result); not a benchmark path. */
int so3_geodesic_eps_f64(const double *R1, const double *R2, double *theta, double *sum, double *result, int mean, double eps,
                         int64_t B, void *stream);

/* ---- K4b: backward of the metrics ----------------------------------------------------------------------------------
 * The reference's three metric spellings are plain differentiable tensor code, and its training loops take any of them as the
 * loss (`lossfunc`: point_cloud/main.py:194-197, UPNA/main.py:56-59; geodesic()'s eps = 1e-7 exists for this gradient,
 * point_cloud/main.py:61-73 and the comment at :64).  With c_b = (sum_ij R1_b,ij R2_b,ij - 1)/2 and
 * theta_b = unit * acos(clamp(c_b, -1 + eps, 1 - eps)) -- tr(R1 R2^T) = tr(R1^T R2), so one formula serves
 * rotation_representation.py:209-227 (eps 0, radians), :230-242 (eps 0, degrees, float64 arithmetic) and geodesic (eps 1e-7) --
 *     dR1_b = h_b R2_b,   dR2_b = h_b R1_b,   h_b = (grad_b / grad_div) * unit * (-1 / sqrt(1 - c_b^2)) / 2
 * for rows with -1 + eps <= c_b <= 1 - eps, and 0 outside the clamp: torch.clamp's / torch.min's / torch.max's backward FILL the
 * gradient with 0 there, the reference never multiplies by acos' infinite slope.  (Divergence: a row with c_b = +-1 EXACTLY
 * and eps = 0 gets -+inf from the reference and 0 here.)  NaN rows give NaN.
 *   R1, R2    in  B*9
 *   grad      in  the upstream gradient d loss / d theta_b: B elements, or ONE element with SO3_GRAD_SCALAR (the 0-dim tensor
 *                 autograd hands to a "mean" / "sum" reduction; a device pointer either way, no host sync).  float32 for
 *                 so3_angle_bwd_f32, float64 with SO3_F64_MATH and for so3_angle_bwd_f64.
 *   grad_div      every gradient element is divided by it first (B for reduction "mean": torch divides, it does not multiply
 *                 by 1/B; 1 otherwise)
 *   eps           the clamp is [-1 + eps, 1 - eps], evaluated in the arithmetic of the spelling (float32 unless SO3_F64_MATH)
 *   dR1, dR2  out B*9 each; either may be NULL (not both)
 *   flags         SO3_RADIANS (default: theta in degrees, as K4), SO3_GRAD_SCALAR, SO3_F64_MATH
 * so3_angle_bwd_f32 without SO3_F64_MATH follows the float32 graph operation for operation (trace summed as so3_geodesic_f32
 * sums it, 1 - c c with both roundings, rsqrt, gradient, mask, / 2, times the other rotation); with it, angle_error's: both
 * rotations cast to float64, every step float64, ONE rounding to float32 at the end.  Streaming engine: 72 B read + 36 B (72 B with
 * both gradients) written per row (+ 4 / 8 B of per-row gradient).  so3_angle_bwd_f64: float64 data, one row per thread. */
int so3_angle_bwd_f32(const float *R1, const float *R2, const void *grad, double grad_div, double eps, unsigned flags,
                      float *dR1, float *dR2, int64_t B, void *stream);
int so3_angle_bwd_f64(const double *R1, const double *R2, const double *grad, double grad_div, double eps, unsigned flags,
                      double *dR1, double *dR2, int64_t B, void *stream);

/* ---- next row: the SE(3) pose update fused after the head ------------------------
 * Replaces calculate_T_pred, Iterative/utility.py:90-128 (the head at :105, einsum at :124, the translation
 * update at :116-121 and the 4x4 assembly the reference's `combine`, :63-71, intends):
 *   dR = proj(out[:, :9]);  R_new = dR R_k;  z_new = vz z_k;  x_new = (vx/fx + x_k/z_k) z_new;  y likewise;
 *   T_pred = [[R_new, (x_new, y_new, z_new)^T], [0, 0, 0, 1]].
 *   out12 in B*12 float32 (network output);  Tinit in B*16 float32 (row-major 4x4);  Tpred out B*16 float32;
 *   fx, fy: focal lengths in pixels (get_scene_parameters, utility.py:73-88: 50 / (36/320) = 444.44).
 * The backward gives dL/dout12 for upstream G = dL/dTpred (B*16); T_init is treated as a constant, as the
 * reference's loop detaches it (Iterative/main.py:97).
 */
int so3_se3_update_f32(const float *out12, const float *Tinit, float *Tpred, float fx, float fy, int64_t B,
                       void *stream);
int so3_se3_update_bwd_f32(const float *out12, const float *Tinit, const float *G, float *dout12, float fx,
                           float fy, int64_t B, void *stream);

/* ---- next row: the 6D Gram-Schmidt head and its backward -------------------------
 * x = a/|a|, z = (x x b)/|x x b|, y = z x x, R = [x y z] as columns; (a, b) = the two halves of each 6-vector.
 * Replaces rotation_representation.py:21-36 (compute_rotation_matrix_from_ortho6d; duplicate at :174-189),
 * the reference's main comparison head (transform_output['6D'], Comparison/models.py:19).
 *   X in B*6 float32;  R out B*9 float32;  G in B*9 float32 (dL/dR);  dX out B*6 float32.
 * No epsilon in the norms, as in the reference: a zero or parallel pair gives Inf/NaN.  Input range: see the heads below.
 */
int so3_ortho6d_fwd_f32(const float *X, float *R, int64_t B, void *stream);
int so3_ortho6d_bwd_f32(const float *X, const float *G, float *dX, int64_t B, void *stream);

/* ---- next row f5: the remaining heads of the reference's dispatch tables -------------
 * Model.func / Model.dimension (Comparison/models.py:18-19, point_cloud/model_fetch.py:153-154), func
 * (3D-Pose/main.py:46,101) and transform_output (rotation_representation.py:323-324) map a key to a head; with
 * these four plus the SVD and 6D heads above every key is served natively ("Direct" is a reshape).
 *   quat     X B*4  (w,x,y,z) -> n = q / max(|q|, 1e-8) -> R(n)      rotation_representation.py:39-50, 137-171
 *   euler    X B*3  R from (c1,s1)=e0, (c2,s2)=e2, (c3,s3)=e1         rotation_representation.py:92-113
 *   ortho5d  X B*5  stereographic un-projection of X[2:5] * (1+sqrt2, 1+sqrt2, sqrt2), then the 6D head
 *                                                                     rotation_representation.py:69-90, 118-134
 *   expmap   X B*3  so(3) exponential map, theta = sqrt(max(|v|^2, 1e-4))   rotation_representation.py:245-275,
 *                   reached as vec_3d_to_SO3 (:309-321, transform_output['3D'])
 * Forward: R out B*9 float32.  Backward: G in B*9 float32 (dL/dR), dX out shaped like X (what the reference
 * gets from autograd through the same formulas).  Degenerate input behaves like the reference's float32 graph
 * (zero 5D tail or zero 6D halves: Inf/NaN), except that an exactly-zero quaternion gives the clamped
 * gradient G-terms/1e-8 where autograd yields NaN.
 *
 * INPUT RANGE OF THE HEADS (tests/heads_ref.py; pinned by tests/test_heads_host.py and tests/test_gpu_heads.py).
 * Inside it every row agrees with the float64 evaluation of the same float32 input within  C u cond,  u = 2^-24,
 * C <= 43 (forward) and <= 31 (backward, in the gradient's own unit: see heads_ref), on the device as on the host:
 *   quat     |q| = 0 and 1e-25 <= |q| <= 1e18.  |q| <= 1e-8 (|q| = 0 too) divides by the constant 1e-8f; q = 0 gives
 *            R = I and a zero gradient.  ABOVE: once |q|^2 overflows (|q| >= 1.9e19) 1/|q| is 0: R = I, gradient 0.
 *   euler    every finite angle (tested to 1e6; sin / cos are the full-range forms, cond = 1).
 *   expmap   every finite v with finite |v|^2; cond = max(1, |v|).  A row within 4 u of |v|^2 = 1e-4 may take
 *            either side of the clamp in its gradient (the forward is continuous there).
 *   ortho6d  each half with 1e-30 <= |.| <= 1e30, independently (the range tested); cond = 1 / sin(a, b).  Both halves
 *            are prescaled by an exact power of two, so neither |a|^2 nor |a x b|^2 = |b|^2 sin^2 overflows or falls
 *            among the subnormals (which v_rsq_f32 reads as 0).  The gradient is of size |G| / (|a| sin), |G| / (|b| sin).
 *            Nothing is promised for subnormal halves or components of 2^127 and above (there the scale itself is
 *            subnormal).  A zero half or parallel halves: Inf / NaN.
 *   ortho5d  X[2:5] and X[0:2] with 1e-10 <= |.| <= 1e10 each (the magnitudes tested); cond = 1 / sin of the
 *            un-projected pair.  BELOW (s = |v|^2 = 0): R[0] = R[3] = 0, every other slot NaN.  ABOVE (s = inf):
 *            every slot NaN.
 * Between the range and those magnitudes a squared norm is subnormal and nothing is promised about the values.
 * In every case the damage stays in its row: a NaN, an inf or an out-of-range row changes no other row.
 */
int so3_quat_fwd_f32(const float *X, float *R, int64_t B, void *stream);
int so3_quat_bwd_f32(const float *X, const float *G, float *dX, int64_t B, void *stream);
int so3_euler_fwd_f32(const float *X, float *R, int64_t B, void *stream);
int so3_euler_bwd_f32(const float *X, const float *G, float *dX, int64_t B, void *stream);
int so3_ortho5d_fwd_f32(const float *X, float *R, int64_t B, void *stream);
int so3_ortho5d_bwd_f32(const float *X, const float *G, float *dX, int64_t B, void *stream);
int so3_expmap_fwd_f32(const float *X, float *R, int64_t B, void *stream);
int so3_expmap_bwd_f32(const float *X, const float *G, float *dX, int64_t B, void *stream);

/* ---- inverse maps (added in 210): rotation matrix -> quaternion, rotation vector, Euler angles; log(R1^T R2) ----
 * The inverses of the quat, expmap and euler heads above.  R in B*9 float32, documented as rotation matrices: nothing is
 * validated on the device, a NaN row gives a NaN row, no input hangs or faults.
 *   mat_to_quat    Q out B*4 (w,x,y,z), the order so3_quat_fwd_f32 reads; unit norm, w >= 0.  Shepperd's method on the
 *                  largest of (tr, r0, r4, r8), branch-free.
 *   logmap         V out B*3, the rotation vector, |v| <= float32(pi) (norm of the float32 result, checked in float64): through the quaternion, theta = 2 atan2(n, w),
 *                  v = (theta / n)(x,y,z) -- no acos of the trace and no (R - R^T) / (2 sin theta), so the axis survives
 *                  next to pi.  Inverse of so3_expmap_fwd_f32 (whose clamp theta^2 >= 1e-4 moves R by less than 1e-7).
 *   mat_to_euler   E out B*3 = (e0, e1, e2) in the euler head's convention (e2 the middle angle):
 *                  (s3, c3) = (r2, r0) / |(r2, r0)| = sincos(e1), e0 = atan2(s3 r3 - c3 r5, c3 r8 - s3 r6),
 *                  e2 = atan2(clamp(-r1, -1, 1), |(r2, r0)|), clamped to the float32 just below pi/2: asin(-r1) for a
 *                  rotation, taken through the two entries that still hold cos(e2) next to gimbal lock (a float32 r1
 *                  rounds to 1 below cos(e2) = 3.5e-4, and asin(-r1) alone then misses R by up to that much).
 *                  GIMBAL LOCK is r0^2 + r2^2, formed in float32, below float32's smallest normal 2^-126 (that is
 *                  |(r2, r0)| below about 1.1e-19, not zero alone: the hardware reciprocal square root reads a subnormal
 *                  as 0).  At gimbal lock cos(e2) = 0 and (s3, c3) = (0, 1): e1 = 0, |e2| is the clamp, e0 =
 *                  atan2(-r5, r8), and the gradient is the floor's.  A NaN row is not at lock: it stays NaN.  |e2| <= pi/2.
 *   relative_log   V out B*3 = log(R1^T R2) in one launch; |v| is the geodesic angle between R1 and R2.
 * GRADIENT CONVENTION.  Every backward returns the TANGENT-SPACE gradient at R: for an inverse map f and the incoming
 * gradient g (G in, shaped like the forward's output) let w = (d f(R exp(hat delta)) / d delta)^T g; then
 *     dR = 1/2 R hat(w)        (dR out B*9 float32),
 * whose inner product with a tangent direction R hat(delta) is w . delta.  It does not depend on the branch the forward
 * took, is bounded for the log map up to theta = pi, and equals the tangent projection R skew(R^T G) of any off-manifold
 * autograd gradient G.  Every head of this library moves R along tangent directions, so chaining through a head is
 * exact.  The Euler gradient carries 1 / cos(e2); cos(e2) is clamped from below at 1e-6 (finite at gimbal lock).
 * so3_relative_log_bwd_f32 writes dR1 and dR2 in one launch; either may be NULL (not both).
 */
int so3_mat_to_quat_fwd_f32(const float *R, float *Q, int64_t B, void *stream);
int so3_mat_to_quat_bwd_f32(const float *R, const float *G, float *dR, int64_t B, void *stream);
int so3_logmap_fwd_f32(const float *R, float *V, int64_t B, void *stream);
int so3_logmap_bwd_f32(const float *R, const float *G, float *dR, int64_t B, void *stream);
int so3_mat_to_euler_fwd_f32(const float *R, float *E, int64_t B, void *stream);
int so3_mat_to_euler_bwd_f32(const float *R, const float *G, float *dR, int64_t B, void *stream);
int so3_relative_log_fwd_f32(const float *R1, const float *R2, float *V, int64_t B, void *stream);
int so3_relative_log_bwd_f32(const float *R1, const float *R2, const float *G, float *dR1, float *dR2, int64_t B, void *stream);

/* ---- row a7: the cloud side of the point-cloud path -------------------------------------
 * so3_rotate_clouds_f32 replaces the pairing rule of the training loop, point_cloud/main.py:173-181
 *   (expand gt_rmat to every point, bmm, view) and, with transposed != 0, the `.transpose(1, 2)` at :183 as well:
 *     P B*N*3, R B*9  ->  out[b][i][:] = R_b p_i   (transposed: out[b][:][i], the (B,3,N) layout the network reads).
 * so3_pc_normalize_f32 replaces pc_normalize, point_cloud/prepare.py:51-56, for a batch of clouds:
 *     centre = (max + min)/2 per axis, scale = |max - min| of the centred cloud, out = (P - centre)/scale;
 *     centroid (B*3) and scale (B) are optional outputs.  float32 (the reference runs it in numpy float64).
 */
int so3_rotate_clouds_f32(const float *P, const float *R, float *out, int transposed, int64_t B, int32_t N, void *stream);
int so3_pc_normalize_f32(const float *P, float *out, float *centroid, float *scale, int64_t B, int32_t N, void *stream);

/* so3_rotate_clouds_bwd_f32 (a7b, added in 210): the backward of so3_rotate_clouds_f32, i.e. the gradient the reference's
 * autograd gives through the bmm of point_cloud/main.py:176-181 (and the transpose at :183) to pc1 and gt_rmat:
 *     dP_bi = R_b^T g_bi,    dR_b = sum_i g_bi p_bi^T,
 *   G        in   B*N*3 float32 upstream gradient in the forward's output layout ((B,N,3), or (B,3,N) with transposed != 0)
 *   dP       out  optional B*N*3 float32 (B,N,3);  dR  out optional B*9 float32 (N == 0 writes dR = 0)
 * P is read only for dR, R only for dP: R must be non-NULL when dP is asked for, P when dR is (and N > 0), G when N > 0.
 * Limits as so3_rotate_clouds_f32.
 */
int so3_rotate_clouds_bwd_f32(const float *P, const float *R, const float *G, float *dP, float *dR, int transposed,
                              int64_t B, int32_t N, void *stream);

/* ---- next row f6: the ADD-L1 losses that consume calculate_T_pred's output, with their gradient ----------------
 * Replaces Iterative/loss.py:10-26 (compute_ADD_L1_loss), :29-48 (compute_disentangled_ADD_L1_loss) and :51-70
 * (transform_pts), called at Iterative/main.py:94-95,150-151,196-197 right after calculate_T_pred, plus the autograd
 * of the loss w.r.t. the predicted pose (which so3_se3_update_bwd_f32 then takes to the network output).
 *   Tgt, Tpred   in  B*16 float32, row-major 4x4 poses
 *   points       in  B*N*3 float32 model points (the reference's `verts`), N >= 1
 *   so3_add_l1_f32:  dist_b = mean over points and coordinates of |T_gt p - T_pred p|
 *     dists      out optional B float32 (use_batch_mean=False);  loss_sum out optional double[1] = sum_b dist_b
 *   so3_add_l1_disentangled_f32:  the three terms of the disentangled loss per sample -- rotation (R_pred with
 *     T_gt's translation), translation x,y and depth z (each with T_gt's rotation; these two do not depend on the
 *     points: the transformed clouds differ by a constant vector)
 *     loss_sum   out double[3] = sum_b (rot_b, transl_b, depth_b);  the reference's value is their total / B
 *   dTpred       out optional B*16 float32: grad_scale * d(sum_b loss_b)/dTpred  (grad_scale = 1/B for the batch
 *                mean; the bottom row is 0; d|x|/dx = sgn(x) with sgn(0) = 0, as autograd)
 * loss_sum is zeroed by the call.  One pass over the points (12 B per point: HBM-read bound).
 */
int so3_add_l1_f32(const float *Tgt, const float *Tpred, const float *points, float *dists, double *loss_sum,
                   float *dTpred, float grad_scale, int64_t B, int32_t N, void *stream);
int so3_add_l1_disentangled_f32(const float *Tpred, const float *Tgt, const float *points, double *loss_sum,
                                float *dTpred, float grad_scale, int64_t B, int32_t N, void *stream);

/* ---- the ADD and ADD-S pose metrics, the ADD-S loss's gradient and the model diameter ---------------------------
 * The numbers a 6-D pose is reported in (Hinterstoisser et al. 2012; PoseCNN's ADD-S); the reference has no such metric.
 * With x_i = R_gt p_i + t_gt and y_j = R_pred p_j + t_pred over the N points of sample b:
 *   so3_add_l2_f32:  ADD_b = (1/N) sum_i |x_i - y_i|_2.  Arguments exactly as so3_add_l1_f32; in dTpred d|e| = e/|e|,
 *     0 where e = 0.
 *   so3_add_s_fwd_f32:  ADDS_b = (1/N) sum_i min_j |x_i - y_j|_2 (the outer sum over the true pose, not symmetric).
 *     point_dist out B*N float32: min_j |x_i - y_j| per point (the work buffer of the row sums: required)
 *     nearest    out optional B*N int32: the argmin j (the first of equal candidates)
 *     dists      out optional B float32: ADDS_b;  loss_sum out optional double[1] = sum_b ADDS_b (written, not added to)
 *   so3_add_s_bwd_f32:  the selected branch's gradient through `nearest` (an index outside [0, N) is clamped):
 *     dTpred out B*16 float32 = grad_scale * grad_rows[b] * dADDS_b/dTpred (grad_rows NULL: 1), bottom row 0
 *   so3_cloud_diameter_f32:  diam_b = max_ij |p_i - p_j|_2;  work: B*N float32 scratch (per-point maxima), diam: B float32
 * Both clouds are posed by the same code and a distance is formed from coordinate differences (never |x|^2 + |y|^2 - 2 x.y),
 * so Tpred == Tgt gives exactly 0 and nearest[i] == i where the points are distinct.  The ADD-S and diameter entries use no
 * atomics: two runs give the same bits.  They are N^2 arithmetic per cloud (compute bound), 1 <= N <= SO3_ADD_S_MAX_N -- so that
 * B*N stays below 2^51 and the 32-bit point and tile indices cannot overflow.
 */
#define SO3_ADD_S_MAX_N 1048576
int so3_add_l2_f32(const float *Tgt, const float *Tpred, const float *points, float *dists, double *loss_sum,
                   float *dTpred, float grad_scale, int64_t B, int32_t N, void *stream);
int so3_add_s_fwd_f32(const float *Tgt, const float *Tpred, const float *points, float *point_dist, int32_t *nearest,
                      float *dists, double *loss_sum, int64_t B, int32_t N, void *stream);
int so3_add_s_bwd_f32(const float *Tgt, const float *Tpred, const float *points, const int32_t *nearest,
                      const float *grad_rows, float grad_scale, float *dTpred, int64_t B, int32_t N, void *stream);
int so3_cloud_diameter_f32(const float *points, float *work, float *diam, int64_t B, int32_t N, void *stream);

/* ---- next row: per-class evaluation statistics on K4's angles ----------------------
 * Replaces the host-side numpy block of 3D-Pose/test_per_class.py:174-216 (np.mean / np.median / np.std / np.max
 * and the accuracy thresholds (x < 30|15|7.5).sum()/len(x)), which the reference feeds one sample at a time.
 *   deg       in  B float64 angles (degrees), e.g. so3_angle_error's per-row output: not negative.  -0.0 counts as +0.0 (in the
 *                 median and the max as in the sums); NEGATIVE angles are outside the contract (they are ordered as 0 but summed
 *                 as they are); +inf and NaN are answered as numpy answers them, see below
 *   cls       in  optional B int32 class ids in [0, ncls) (NULL: one class); rows with other ids are ignored
 *   stats     out ncls x 8 doubles: count, mean, std (population, as np.std), max, median (EXACT: radix select
 *                 on the float64 bits, the two middle elements averaged as np.median does), acc<30, acc<15, acc<7.5.
 *                 std is the one-pass sqrt(S2/m - (S1/m)^2) over float64 sums: |std^2 - np.var(x)| <= c D 2^-53 (mean(x^2) + mean(x)^2),
 *                 D = B / (8 x workgroups) + workgroups + 49 the additions a row's value passes (workgroups = min(ceil(B/2048),
 *                 CUs)), c = 0.13 (never above 2 and a little) -- about 1e-11 deg^2 at a million rows of tens
 *                 of degrees: a distribution whose std is below ~1e-7 of its mean gets no correct digit of it (0 where the
 *                 difference comes out negative).
 *                 An EMPTY class reports count 0 and NaN in every other field.  A class holding +inf reports mean = max = +inf,
 *                 std = NaN and numpy's median.
 *   workspace     caller-owned scratch of so3_angle_stats_workspace_bytes() bytes (~10 MB: histograms and a buffer for the
 *                 candidates of the medians), ZERO-FILLED ONCE before its first use -- every call leaves its sums and histograms
 *                 zeroed and re-initialises its control words in its first launch --, used by ONE stream at a time (re-zero it
 *                 after a call that returned an error).  A call whose launches are delayed by other work on the device (its
 *                 workgroups wait for each other, boundedly) is slower, never wrong, and leaves the workspace as usable as before.
 * ncls <= 64.  A class containing a NaN angle reports NaN for mean/std/max/median, as numpy does.
 * Two launches, two passes over the rows: a histogram pass, and a pass that compacts the rows of the medians' 1/16-octave bins and
 * then, one workgroup per class behind a ticket, selects among them.
 */
size_t so3_angle_stats_workspace_bytes(void);
int so3_angle_stats(const double *deg, const int32_t *cls, int32_t ncls, double *stats, void *workspace,
                    int64_t B, void *stream);

/* ---- K5: fused Kabsch (config #3) ------------------------------------------------------------------
 * H_b = sum_i q_bi p_bi^T (= bmm(Q^T, P)),  R_b = proj_SO(3)(H_b) = argmin_R sum_i |R p_bi - q_bi|^2.
 * No centring: the reference's pairing rule q = R p has no translation (point_cloud/main.py:173-181).
 * The reference has no closed-form solve (it learns R with PointNet++); the oracle is
 * symmetric_orthogonalization(bmm(Q^T, P)).
 *   P, Q in  B*N*3 float32, cloud-major then point-major (the (B,1024,3) tensors of
 *            point_cloud/main.py:171);  R out B*9 float32;  H out optional B*9 float32.
 */
int so3_kabsch_f32(const float *P, const float *Q, float *R, float *H, int64_t B, int32_t N,
                   void *stream);

/* ---- K5b: Kabsch backward (added in 210) ----------------------------------------------------------------
 * The gradient the reference's autograd gives through symmetric_orthogonalization(bmm(Q^T, P))
 * (rotation_representation.py:192-206 after the pairing rule of point_cloud/main.py:176-181), given the forward's H:
 *     dH = K2(H, gR) + gH,    dQ_bi = dH_b p_bi,    dP_bi = dH_b^T q_bi.
 * K2 is so3_project_bwd_f32's closed form, with its singular denominators clamped (a planar cloud's H is still
 * fine; a collinear or all-zero cloud gets a finite gradient where autograd's is Inf / NaN).
 *   P, Q     in   B*N*3 float32 (as for so3_kabsch_f32; dQ reads only P, dP reads only Q)
 *   H        in   B*9 float32, the H so3_kabsch_f32 returned for P, Q
 *   gR, gH   in   optional B*9 float32 upstream gradients of R and H (NULL: zero)
 *   dP, dQ   out  optional B*N*3 float32 (NULL: not computed; a one-sided call reads half the bytes)
 * Limits and NULL rules as so3_kabsch_f32: H always, P and Q when N > 0.  One launch, no atomics.
 */
int so3_kabsch_bwd_f32(const float *P, const float *Q, const float *H, const float *gR, const float *gH,
                       float *dP, float *dQ, int64_t B, int32_t N, void *stream);

/* ---- K5c / K5d: rigid_align, the weighted and centred Kabsch giving a pose (added in 210) -------------------
 * For every cloud b, with weights w_i >= 0 (all ones when w is NULL):
 *     W = sum w_i,   pbar = sum w_i p_i / W,   qbar = sum w_i q_i / W,
 *     H = sum w_i (q_i - qbar)(p_i - pbar)^T        (not divided by W: the projection is scale-free)
 *     R = proj_SO(3)(H),   t = qbar - R pbar        = argmin over (R, t) of sum w_i |R p_i + t - q_i|^2.
 * W == 0 (all weights zero, or N == 0): pbar = qbar = 0, H = 0, R = I, t = 0, and every gradient is 0; nothing divides
 * by W unguarded.  Negative weights are undefined and not checked.  NaN in -> NaN out, and a point of weight 0 must
 * still be finite (0 * Inf is NaN).
 * One pass over the clouds.  The sums are taken relative to a pivot, the cloud's FIRST point pair (p_0, q_0), whatever
 * its weight, so that float32 keeps its digits however far from the origin the clouds lie: R is as accurate as for
 * centred clouds, t to eps * |qbar|.  That assumes the pivot lies within the cloud's extent: padding a cloud with
 * junk is fine, putting junk far outside the cloud FIRST is not.
 *   P, Q   in   B*N*3 float32, as for so3_kabsch_f32
 *   w      in   optional B*N float32
 *   R, t   out  B*9, B*3 float32
 *   H      out  optional B*9 float32
 *   stats  out  optional B*7 float32: pbar (3), qbar (3), W -- what the backward needs besides H and R
 * so3_rigid_align_bwd_f32: given the forward's H, R and stats, and upstream gradients gR, gt, gH (each optional: zero),
 * with a_i = p_i - pbar, c_i = q_i - qbar, u = R^T gt:
 *     dH = K2(H, gR - gt pbar^T) + gH
 *     dQ_i = w_i dH a_i + (w_i / W) gt,   dP_i = w_i dH^T c_i - (w_i / W) u,   dw_i = c_i^T dH a_i + (gt . c_i - u . a_i) / W.
 *   dP, dQ out optional B*N*3 float32, dw out optional B*N float32 (NULL: not computed; dQ alone reads only P and w, dP
 *   alone only Q and w).  w may be NULL (all ones), and dw may still be asked for.  K2's clamp applies where H has a
 *   vanishing singular-value gap, as for so3_kabsch_bwd_f32.  One launch each, no atomics, no host synchronisation.
 * Limits as so3_kabsch_f32; R and t (forward), H, R and stats (backward) always, P and Q when N > 0.
 */
int so3_rigid_align_f32(const float *P, const float *Q, const float *w, float *R, float *t, float *H, float *stats,
                        int64_t B, int32_t N, void *stream);
int so3_rigid_align_bwd_f32(const float *P, const float *Q, const float *w, const float *H, const float *R,
                            const float *stats, const float *gR, const float *gt, const float *gH, float *dP, float *dQ,
                            float *dw, int64_t B, int32_t N, void *stream);

/* ---- nearest neighbours between two clouds, and ICP (iterative closest point) on top of them (added in 210) ----
 * so3_nearest_f32: for every point x_i of cloud b (N points) the closest of the M points of its target cloud,
 *     dist[b][i] = min_j |x_i - y_j|_2,   nearest[b][i] = the argmin j (the first of equal candidates).
 *   X        in   B*N*3 float32
 *   Y        in   the targets; y_stride = floats between two clouds' targets: 0 for ONE target shared by the batch
 *                 (M*3 float32), otherwise >= 3*M (B*M*3 float32 packed: 3*M)
 *   dist     out  B*N float32 (required);  nearest out optional B*N int32
 *   Distances come from coordinate differences (never |x|^2 + |y|^2 - 2 x.y): a point of X that is also in Y gets exactly 0.
 * so3_icp_f32: `iterations` ICP iterations from the pose T_init, without early exit.  One iteration from (R_k, t_k):
 *     x_i = R_k p_i + t_k;   j(i), d_i as so3_nearest_f32(x, Q);   w'_i = w_i * [d_i <= max_distance];
 *     (R_k+1, t_k+1) = so3_rigid_align_f32's answer for the pairs (p_i, q_j(i)) with weights w' -- from the UNPOSED p_i, so
 *     the result is an absolute pose and no composition error builds up; the pivot of the sums is (p_0, q_0), the first
 *     source and the first target point;
 *     rmse[k][b] = sqrt(sum w' d^2 / sum w'),   inliers[k][b] = #{i : w'_i > 0}   -- both at the pose the iteration started from.
 *   sum w' == 0 leaves the pose as it was, with rmse 0 and inliers 0.  iterations == 0 returns the initial pose (and, when
 *   asked for, nearest and dist of a search at that pose).
 *   P        in   B*N*3 float32, the source clouds;   Q, q_stride: the targets, as Y, y_stride above (M points)
 *   w        in   optional B*N float32 weights >= 0 (NULL: all ones)
 *   T_init   in   optional B*12 float32: per cloud the rows (R | t) of the initial pose, [4c .. 4c+2] = row c of R,
 *                 [4c+3] = t_c (NULL: the identity)
 *   max_distance  < 0: no trimming
 *   R, t     out  B*9, B*3 float32: the pose after the last iteration
 *   rmse     out  optional iterations*B float32;   inliers out optional iterations*B int32
 *   nearest, dist  out optional B*N int32 / float32: the LAST iteration's search (at the pose that iteration started from)
 *   workspace     caller-owned, so3_icp_workspace_bytes(B, N) bytes (0 for B or N out of range), 16-byte aligned.  It needs
 *                 no zero-fill: the call writes every word before it reads it.
 * An iteration is two launches on the caller's stream; nothing synchronises with the host and nothing uses atomics, so a
 * call can be captured in a graph and the same inputs give the same bits.  1 <= N, M <= SO3_ADD_S_MAX_N,
 * 0 <= iterations <= SO3_ICP_MAX_ITERATIONS.  Not differentiable: for gradients call so3_rigid_align_f32 / _bwd_f32 on
 * the returned correspondences.
 */
#define SO3_ICP_MAX_ITERATIONS 1000
int so3_nearest_f32(const float *X, const float *Y, int64_t y_stride, float *dist, int32_t *nearest, int64_t B, int32_t N,
                    int32_t M, void *stream);
size_t so3_icp_workspace_bytes(int64_t B, int32_t N);
int so3_icp_f32(const float *P, const float *Q, int64_t q_stride, const float *w, const float *T_init, float max_distance,
                int32_t iterations, float *R, float *t, float *rmse, int32_t *inliers, int32_t *nearest, float *dist,
                void *workspace, int64_t B, int32_t N, int32_t M, void *stream);

/* ---- point-to-plane ICP over the target's normals (added in 210) ----
 * so3_icp_plane_f32: `iterations` Gauss-Newton iterations of  min sum_i w'_i (n_j(i) . (R p_i + t - q_j(i)))^2  from the pose
 * T_init, without early exit.  One iteration from m_k = (R_k | t_k), for cloud b:
 *   1. search   x_i = pose_point(m_k, p_i);  j(i), d2_i, d_i = sqrt(d2_i) exactly as so3_nearest_f32(x, Q): nearest and dist are
 *               the bits so3_icp_f32 returns from the same pose.
 *   2. normal   n_i = normals[b][j(i)]; the normals lie beside Q with the same stride (q_stride == 0: one shared target and one
 *               shared normal array); j is clamped to M - 1 before anything is addressed.  A normal whose three components are
 *               all zero names no plane (so3_local_frames_f32's rows past a length, a flat patch).
 *   3. weight   w'_i = w_i * [d_i <= max_distance] * [n_i != 0]   (max_distance < 0: no trimming).
 *   4. row      pivot c = pose_point(m_k, p_0), the posed first source point: moments are taken about a point inside the
 *               cloud, so a cloud 100 units from the origin keeps float32's digits.  a_i = x_i - c, e_i = x_i - q_j(i) (one
 *               rounded subtraction per coordinate), r_i = n_i . e_i, J_i = (a_i x n_i, n_i) in R^6.
 *   5. sums     sum w';  the 21 upper-triangle entries of A = sum w' J J^T;  g = sum w' J r;  sum w' r^2;  sum w' d2;  the
 *               count #{w' > 0}: 31 sums per work item in a record of 32 floats, added in a fixed order (no atomics).
 *   6. finish   sum w' == 0: not live -- the pose is kept, both rmse are 0, solved = 0.  Otherwise A'_aa = A_aa (1 + damping)
 *               (Levenberg-Marquardt's diagonal form) and a 6x6 Cholesky A' = L L^T in float32; pivot k passes when
 *               p_k > SO3_ICP_PLANE_PIVOT_EPS * A'_kk (strictly: an exactly zero column fails).  Any failed pivot: the cloud
 *               is UNSOLVED -- the pose is kept, solved = 0, rmse and inliers are still reported.  With damping > 0 a column
 *               with A_kk == 0 (J_k = 0 on every inlier, so its row, its column and g_k are 0 as well) is skipped with
 *               delta_k = 0 instead of failing: scaling a zero diagonal cannot lift it, and 0 is the limit of Marquardt's
 *               additive form.  SO3_ICP_PLANE_PIVOT_EPS is the largest power of two at which the float32 arithmetic solves
 *               every step of the test fixture whose float64 equilibrated condition number is at most 1e3.  Otherwise
 *               delta = -A'^-1 g, omega = delta[0:3], v = delta[3:6];  with h = omega / 2, s = |h|^2:
 *                   dR = I + (2 / (1 + s)) (hat(h) + hat(h)^2)       -- the rotation of the quaternion (1, h), no sin / cos,
 *                   R_k+1 = so3_project_fwd_f32's projection of dR R_k,   t_k+1 = dR (t_k - c) + c + v.
 *               rmse[k][b] = sqrt(sum w' r^2 / sum w') (point-to-plane), rmse_point[k][b] = sqrt(sum w' d2 / sum w'),
 *               inliers[k][b] = the count -- all at the pose the iteration started from.
 * Negating any of the normals changes no bit of any output (r and J flip together), so no orientation step is needed.
 *   P, Q, q_stride, w, T_init, max_distance, R, t, nearest, dist: as so3_icp_f32
 *   normals     in   as Q: M*3 float32 per target (B of them, or one with q_stride == 0)
 *   damping     >= 0 (negative or NaN: invalid argument); 0 is plain Gauss-Newton
 *   rmse, rmse_point  out optional iterations*B float32;   inliers, solved  out optional iterations*B int32
 *   workspace   caller-owned, so3_icp_plane_workspace_bytes(B, N) bytes (0 for B or N out of range), 16-byte aligned; no zero-fill.
 * iterations == 0 returns the initial pose (and, when asked for, nearest and dist of a search at that pose).  An iteration is
 * two launches on the caller's stream; nothing synchronises with the host and nothing uses atomics or memset, so a call can be
 * captured in a graph, the same inputs give the same bits, and a NaN or Inf cloud changes no other cloud.  Limits as
 * so3_icp_f32.  Not differentiable.
 */
#define SO3_ICP_PLANE_PIVOT_EPS 0.0078125f /* 2^-7 */
size_t so3_icp_plane_workspace_bytes(int64_t B, int32_t N);
int so3_icp_plane_f32(const float *P, const float *Q, const float *normals, int64_t q_stride, const float *w,
                      const float *T_init, float max_distance, float damping, int32_t iterations, float *R, float *t,
                      float *rmse, float *rmse_point, int32_t *inliers, int32_t *solved, int32_t *nearest, float *dist,
                      void *workspace, int64_t B, int32_t N, int32_t M, void *stream);

/* ---- Chamfer distance between two ragged clouds, with gradients to both (added in 210) ----
 * Cloud b uses the first n_b = clip(x_len[b], 0, N) points of X and the first m_b = clip(y_len[b], 0, M) points of Y (NULL: all).
 *     j(i) = the first argmin over j < m_b of |x_i - y_j|^2,   i(j) = the first argmin over i < n_b of |y_j - x_i|^2
 *     (so3_nearest_f32's search: coordinate differences, strict < in ascending index; a point in both clouds gets exactly 0),
 *     e = d^2, or d with SO3_CHAMFER_UNSQUARED (one square root after the minimum),
 *     rows[b] = (sum_{i<n_b} e_i / n_b,  sum_{j<m_b} e_j / m_b);  with SO3_CHAMFER_SINGLE only the x direction runs and rows[b][1] = 0.
 *   A cloud with n_b == 0 or m_b == 0 scores (0, 0) and takes no gradient.  A slot past its cloud's length reads dist 0,
 *   nearest -1 and a gradient row of zeros: every element of every output is written, no buffer needs a zero-fill.
 * so3_chamfer_fwd_f32: one launch searches both directions, a second adds each cloud's partial sums in a fixed order (float64).
 *   X, Y           in   B*N*3, B*M*3 float32;   x_len, y_len  in  optional B int32
 *   dist_x, dist_y out  optional B*N, B*M float32: the per-point e;   nearest_x, nearest_y  out  optional B*N, B*M int32
 *                       (dist_y and nearest_y must be NULL with SO3_CHAMFER_SINGLE)
 *   rows           out  B*2 float32 (required)
 *   work                caller-owned, so3_chamfer_workspace_bytes(B, N, M) bytes (0 out of range), 4-byte aligned, no zero-fill
 * so3_chamfer_bwd_f32: one launch, both gradients as a gather through the two index arrays the forward left:
 *     dX[b][i] = scale_x[b] phi(x_i - y_j(i)) + sum_{j < m_b, i(j) = i} scale_y[b] phi(x_i - y_j),   dY the mirror image,
 *     phi(v) = 2 v, or v / |v| (0 at v = 0) with SO3_CHAMFER_UNSQUARED;
 *   per coordinate one chain: the own term (a rounded product), then fma(scale, phi, acc) over the hits in ascending index.
 *   scale_x, scale_y  in  B float32: the upstream gradient of rows[b][0], rows[b][1] times the reduction's 1 / n_b, 1 / m_b.
 *   With SO3_CHAMFER_SINGLE nearest_y and scale_y must be NULL (dY then holds the x direction's hits alone); otherwise both are
 *   required.  dX, dY  out  B*N*3, B*M*3 float32, each optional, not both NULL.
 * Nothing synchronises with the host and nothing uses atomics: a call can be captured in a graph and the same inputs give the
 * same bits.  1 <= N, M <= SO3_ADD_S_MAX_N, B as so3_nearest_f32 (0: a no-op).
 */
#define SO3_CHAMFER_UNSQUARED 1u
#define SO3_CHAMFER_SINGLE 2u
size_t so3_chamfer_workspace_bytes(int64_t B, int32_t N, int32_t M);
int so3_chamfer_fwd_f32(const float *X, const float *Y, const int32_t *x_len, const int32_t *y_len, float *dist_x,
                        int32_t *nearest_x, float *dist_y, int32_t *nearest_y, float *rows, void *work, uint32_t flags, int64_t B,
                        int32_t N, int32_t M, void *stream);
int so3_chamfer_bwd_f32(const float *X, const float *Y, const int32_t *x_len, const int32_t *y_len, const int32_t *nearest_x,
                        const int32_t *nearest_y, const float *scale_x, const float *scale_y, float *dX, float *dY,
                        uint32_t flags, int64_t B, int32_t N, int32_t M, void *stream);

/* ---- Chamfer's normal term: the cosine loss on the nearest pairs, with gradients to both normal sets (added in 210) ----
 * Lengths, the two searches, nearest_x, nearest_y, dist_x, dist_y and rows are so3_chamfer_fwd_f32's, bit for bit, on the same
 * input.  NX (B*N*3) and NY (B*M*3) hold a normal per point; they need not be of unit length.  Each direction pairs a point's own
 * normal a with the normal b of the point its search returned: direction x pairs nx_i with ny_j(i), direction y ny_j with nx_i(j).
 *     saa = a.a, sbb = b.b, sab = a.b, each one fused multiply-add chain in x, y, z order;
 *     ra = rsq(saa), rb = rsq(sbb), c = (sab ra) rb;
 *     a pair is FLAT when !(saa > 0 && saa < inf && sbb > 0 && sbb < inf) -- a zero, NaN or infinite normal, a length whose square
 *     leaves float32's range: c = 0, the term is 1 and NEITHER normal takes a gradient from the pair;
 *     t = 1 - |c|, or 1 - c with SO3_CHAMFER_SIGNED_COSINE; t is not clamped (parallel normals may give a t a few ulp below 0);
 *     rows_n[b] = (sum_{i<n_b} t_i / n_b, sum_{j<m_b} t_j / m_b), the records, float64 chunk-order sums and division of rows;
 *     (0, 0) for a cloud with an empty side, a second entry of 0 with SO3_CHAMFER_SINGLE.
 *   rsq is a 1-ulp instruction and not part of the definition: term_*, rows_n, dNX and dNY are defined up to it.
 * so3_chamfer_normals_fwd_f32: so3_chamfer_fwd_f32's two launches with the term formed behind the search.
 *   X, Y, NX, NY   in   required;   x_len, y_len  in  optional B int32
 *   dist_*, nearest_*   out  optional, as so3_chamfer_fwd_f32;   term_x, term_y  out  optional B*N, B*M float32: the per-point t,
 *                       0 in a slot past its cloud's length (dist_y, nearest_y and term_y must be NULL with SO3_CHAMFER_SINGLE)
 *   rows, rows_n   out  B*2 float32 each (required)
 *   work                caller-owned, so3_chamfer_normals_workspace_bytes(B, N, M) bytes (0 out of range), 4-byte aligned, no zero-fill
 * so3_chamfer_normals_bwd_f32: one launch, both gradients as a gather through the two index arrays the forward left:
 *     psi(a, b) = dt/da = -sigma ra (b rb - c a ra),  sigma = sgn(c) in {-1, 0, +1}, or 1 with SO3_CHAMFER_SIGNED_COSINE; 0 for a flat pair;
 *     dNX[b][i] = scale_x[b] psi(nx_i, ny_j(i)) + sum_{j < m_b, i(j) = i} scale_y[b] psi(nx_i, ny_j),   dNY the mirror image
 *   (t is symmetric in a and b: both uses of a normal take psi with the owner first).  Per coordinate one chain: the own term (a
 *   rounded product), then fma(scale, psi, acc) over the hits in ascending index.  The term gives no gradient to X or Y: the indices
 *   are piecewise constant.  scale_x, scale_y  in  B float32: the upstream gradient of rows_n[b][0], rows_n[b][1] times 1 / n_b, 1 / m_b.
 *   With SO3_CHAMFER_SINGLE nearest_y and scale_y must be NULL (dNY then holds the x direction's hits alone); otherwise both are
 *   required.  dNX, dNY  out  B*N*3, B*M*3 float32, each optional, not both NULL; a padded slot gets a row of zeros.
 *   flags: SO3_CHAMFER_UNSQUARED (the forward's e), SO3_CHAMFER_SINGLE, SO3_CHAMFER_SIGNED_COSINE.
 * Every element of every output is written.  Nothing synchronises with the host and nothing uses atomics or a zero-fill: a call
 * can be captured in a graph and the same inputs give the same bits.  Limits and the B == 0 no-op as so3_chamfer_fwd_f32.
 */
#define SO3_CHAMFER_SIGNED_COSINE 4u
size_t so3_chamfer_normals_workspace_bytes(int64_t B, int32_t N, int32_t M);
int so3_chamfer_normals_fwd_f32(const float *X, const float *Y, const float *NX, const float *NY, const int32_t *x_len,
                                const int32_t *y_len, float *dist_x, int32_t *nearest_x, float *dist_y, int32_t *nearest_y,
                                float *term_x, float *term_y, float *rows, float *rows_n, void *work, uint32_t flags, int64_t B,
                                int32_t N, int32_t M, void *stream);
int so3_chamfer_normals_bwd_f32(const float *NX, const float *NY, const int32_t *x_len, const int32_t *y_len,
                                const int32_t *nearest_x, const int32_t *nearest_y, const float *scale_x, const float *scale_y,
                                float *dNX, float *dNY, uint32_t flags, int64_t B, int32_t N, int32_t M, void *stream);

/* ---- K nearest neighbours between two ragged clouds, with gradients to both (added in 210) ----
 * Cloud b uses the first n_b = clip(x_len[b], 0, N) points of X and the first m_b = clip(y_len[b], 0, M) points of Y (NULL: all).
 * The arithmetic is a definition, not an approximation:
 *     d(i, j) = ((dx * dx) + (dy * dy)) + (dz * dz) from coordinate differences, every operation rounded to float32 on its own, no
 *     fused multiply-add (so3_three_nn_f32's and so3_fps_f32's distance);
 *     row i < n_b holds the r = min(K, m_b) smallest candidates j < m_b, ordered "smaller d first, among equal d the lower j first":
 *     dist2[b][i][k] = d, idx[b][i][k] = j.
 *   dist2 = 0 and idx = -1 fill every slot k >= r, every slot of a row i >= n_b, every slot of a cloud with m_b == 0, and a slot that
 *   never received a candidate (non-finite coordinates only: a NaN or +inf d fails every <).  Every element of both outputs is
 *   written; no buffer needs a zero-fill.  so3_group_points_f32 reads -1 as an empty slot.
 *   K = 3 with full lengths and M >= 3 gives so3_three_nn_f32's dist2 and idx bit for bit.  K = 1 gives the first argmin of THIS d,
 *   which is not necessarily so3_nearest_f32's: that search forms d with fused multiply-adds, and two candidates within rounding of
 *   each other can change places between the two forms.
 * so3_knn_f32: one launch.
 *   X        in   B*N*3 float32;   Y  in  cloud b's target at Y + b*y_stride floats (y_stride 0: one target shared by all clouds,
 *                 otherwise >= 3*M), as so3_nearest_f32;   x_len, y_len  in  optional B int32
 *   dist2    out  optional B*N*K float32;   idx  out  B*N*K int32 (required)
 * so3_knn_bwd_f32: one launch, the gradient of dist2 to both clouds as a gather through idx (per-cloud targets: Y is B*M*3).
 *   Per coordinate c one chain from +0, the difference one rounded subtraction, the doubling exact:
 *     dX[b][i][c]: over k = 0 .. r-1 ascending,  acc = fma(g[b][i][k], 2 (x_ic - y_jc), acc)  with j = idx[b][i][k];
 *     dY[b][j][c]: over the entries (i, k), i < n_b, with idx[b][i][k] == j, in ascending (i, k),  acc = fma(g[b][i][k], 2 (y_jc - x_ic), acc).
 *   A padded slot (-1) contributes nothing.  idx holds -1 or values in [0, m_b); anything else reads nothing out of bounds (dX clamps
 *   it into [0, m_b), dY ignores it).  Rows i >= n_b of
 *   dX and j >= m_b of dY, and both gradients of a cloud with n_b == 0 or m_b == 0, are written as zeros.
 *   idx, grad_dist2  in  B*N*K;   dX, dY  out  B*N*3, B*M*3 float32, each optional, not both NULL.
 * Nothing synchronises with the host and nothing uses atomics: a call can be captured in a graph and the same inputs give the
 * same bits.  1 <= K <= SO3_KNN_MAX_K (K > M is legal), 1 <= N, M <= SO3_ADD_S_MAX_N, B as so3_nearest_f32 (0: a no-op).
 * B, N, M and K are checked first: B == 0 with a K out of range is an error, B == 0 with NULL pointers is not.
 */
#define SO3_KNN_MAX_K 64
int so3_knn_f32(const float *X, const float *Y, int64_t y_stride, const int32_t *x_len, const int32_t *y_len, float *dist2,
                int32_t *idx, int32_t K, int64_t B, int32_t N, int32_t M, void *stream);
int so3_knn_bwd_f32(const float *X, const float *Y, const int32_t *x_len, const int32_t *y_len, const int32_t *idx,
                    const float *grad_dist2, float *dX, float *dY, int32_t K, int64_t B, int32_t N, int32_t M, void *stream);

/* ---- Local frames: per-point PCA over a neighbourhood given by indices (added in 210) ----
 * For every row of idx (so3_knn_f32's, so3_ball_query_f32's or a caller's own): the 3x3 covariance of the points it names, its
 * eigenvalues and a right-handed frame of its eigenvectors; the first column is the surface normal.  One launch.
 * Cloud b is at Y + b*y_stride floats (0: one cloud shared by all, otherwise >= 3*M), as so3_knn_f32; rows i < n_b =
 * clip(x_len[b], 0, N) are live and points j < m_b = clip(y_len[b], 0, M) exist (NULL: all).
 * A slot of row (b, i) is VALID when 0 <= idx < m_b (one unsigned compare); every other value -- the -1 padding, an empty ball's
 * N, garbage -- is skipped and addresses nothing.  Valid slots need not form a prefix.  r = the number of valid slots, j_0 = the
 * first valid one, the pivot.
 * The covariance is a definition, not an approximation (float32, bit-exact):
 *     d_k = y_{j_k} - y_{j_0} per coordinate, one rounded subtraction each;
 *     s = sum_k d_k, a chain of rounded additions from +0 over the valid slots in ascending k;   m = s / (float)r, IEEE division;
 *     e_k = d_k - m;   for (xx, xy, xz, yy, yz, zz): S_ab a chain from +0 in ascending k of fma(e_ka, e_kb, S_ab);   C_ab = S_ab / (float)r.
 *   Centring on the pivot keeps float32's digits however far from the origin the cloud lies; scaling the cloud by a power of two
 *   scales C by its square, bit for bit.
 * The eigen stage is an approximation with bounds (tests/local_frames_ref.py): eigenvalues l0 <= l1 <= l2, each >= 0, and unit
 * eigenvectors e0, e1, e2.  C is prescaled by an exact power of two, so scaling the cloud by 2^k leaves the frame's bits unchanged
 * and multiplies the eigenvalues by 4^k exactly.  A fixed number of Jacobi sweeps: no loop bound depends on the data.
 * Signs: in e0 and in e2 the component of largest magnitude is positive (among equal magnitudes the lowest index decides); with a
 * viewpoint v_b, e0 is then flipped where e0 . (v_b - y_{j_0}) < 0 (exactly 0 keeps the sign); then e1 = e2 x e0 (det = +1).
 * C == 0 exactly (r = 1, all neighbours equal) gives eigenvalues 0 and the identity frame, with or without a viewpoint.  Rows with r = 0, rows i >= n_b and every
 * row of a cloud with m_b = 0 are written as zeros in every output.  Every element of every requested output is written; no buffer
 * needs a zero-fill.  Non-finite coordinates give unspecified values in the rows that name them only.
 *   Y            in   the clouds, float32;   idx  in  B*N*K int32;   x_len, y_len  in  optional B int32
 *   viewpoint    in   optional B*3 float32
 *   cov          out  B*N*6 float32  (xx, xy, xz, yy, yz, zz)
 *   eigenvalues  out  B*N*3 float32  l0, l1, l2
 *   normals      out  B*N*3 float32  e0
 *   frames       out  B*N*9 float32  row-major 3x3, columns e0 e1 e2
 *   each output optional, not all NULL.
 * No atomics, no workspace, no host synchronisation: a call can be captured in a graph and the same inputs give the same bits.
 * 1 <= K <= SO3_KNN_MAX_K, N, M, B as so3_knn_f32 (B == 0: a no-op).  B, N, M and K are checked first: B == 0 with a K out of
 * range is an error, B == 0 with NULL pointers is not.
 */
int so3_local_frames_f32(const float *Y, int64_t y_stride, const int32_t *idx, const int32_t *x_len, const int32_t *y_len,
                         const float *viewpoint, float *cov, float *eigenvalues, float *normals, float *frames, int32_t K, int64_t B,
                         int32_t N, int32_t M, void *stream);

/* ---- FPFH: Fast Point Feature Histograms over a cloud's own neighbourhoods (added in 210) ----
 * The descriptor of Rusu et al. 2009 as PCL and Open3D ship it: 33 floats per point that a rigid motion of the cloud leaves alone.
 * Two launches: so3_spfh_f32 builds every point's simplified histogram (SPFH) over its row of idx, so3_fpfh_f32 adds the distance-
 * weighted mean of the neighbours' histograms.  The queries are the cloud's own points: row i of idx (B*N*K) is point i's
 * neighbourhood in the same cloud.  Cloud b has n_b = clip(len[b], 0, N) points (NULL: all).  Normals are used as given; unit length is
 * a precondition.
 * PAIR.  Slot k of row (b, i) with j = idx[b,i,k] is a pair when all of these hold:
 *     0 <= j < n_b (one unsigned compare);   j != i;
 *     dp = p_j - p_i (one rounded subtraction per coordinate) has d2 = fma(dp_z, dp_z, fma(dp_y, dp_y, dp_x * dp_x)) > 0;
 *     neither n_i nor n_j has all three components zero (so3_icp_plane_f32's rule);
 *     |dp x n1|^2 > 0 after the choice of roles below;   none of the three features is NaN.
 *   A row is a multiset: an index that stands twice counts twice (so3_ball_query_f32 pads with its first hit; a caller who wants a set
 *   overwrites that padding with -1).  No index addresses anything before it is tested.
 * FEATURES.  d = sqrt(d2), a1 = (n_i . dp) / d, a2 = (n_j . dp) / d.  If |a1| < |a2| (strictly) the roles swap: n1 = n_j, n2 = n_i,
 *   dp <- -dp, f3 = -a2; otherwise n1 = n_i, n2 = n_j, f3 = a1.  v = (dp x n1) / |dp x n1|, w = n1 x v, f2 = v . n2,
 *   f1 = atan2(w . n2, n1 . n2).
 * BINS.  h(g) = min(10, max(0, (int)floor(g))) with g1 = 11 (f1 + pi) / (2 pi), g2 = 11 (f2 + 1) / 2, g3 = 11 (f3 + 1) / 2; the
 *   histogram's 33 slots are [h(g1) | 11 + h(g2) | 22 + h(g3)].  The arithmetic that produces g is NOT part of the bit contract
 *   (reciprocal square roots, a polynomial atan2 and contraction are free): the counts are, for inputs whose g stay clear of the
 *   integers (tests/fpfh_ref.py: the margin condition).
 * SPFH.  pairs[b,i] = r, the number of pairs of the row; spfh[b,i,s] = (100 c_s) / (float)r with c_s the integer count of slot s:
 *   100 c_s is exact and the division is IEEE, so spfh is bit-exact given the counts.  Each of the three sub-histograms sums to 100.
 *   r = 0, rows i >= n_b and clouds with n_b = 0 are written as zeros.
 * FPFH is a definition, bit for bit (float32; the fusions are the fmas spelled out, divisions are IEEE).  For slot k in ascending
 *   order with 0 <= j < n_b, j != i and d2 > 0:   w = 1 / d2;   the slot is used when w < inf and pairs[b,j] > 0;
 *       W <- W + w, a rounded chain from +0;     A_s <- fma(w, spfh[b,j,s], A_s), from +0;
 *   then fpfh[b,i,s] = spfh[b,i,s] + (W > 0 ? A_s / W : 0).  Every neighbour's sub-histogram sums to 100, so W is the normaliser
 *   Open3D obtains by summing bins: each sub-histogram of fpfh sums to 200 up to rounding (100 or 0 where a side is empty).
 *   Rows i >= n_b are written as zeros.  w < inf does not keep A_s finite: from about w = 2^121 a spfh of 100 overflows the fma, and
 *   the defined result is then inf or NaN.
 * Scaling the cloud by a power of two leaves pairs, spfh and fpfh bit-identical (within float32's range).  A NaN or infinite point or
 * normal changes only the rows that name it (for fpfh: and the rows that name those).  Every element of every requested output is
 * written; no buffer needs a zero-fill.  No atomics, no workspace, no host synchronisation: the calls can be captured in a graph and
 * the same inputs give the same bits.
 *   X, normals  in   B*N*3 float32;   idx  in  B*N*K int32;   len  in  optional B int32
 *   spfh        out (so3_spfh_f32) / in (so3_fpfh_f32)   B*N*33 float32
 *   pairs       out (so3_spfh_f32) / in (so3_fpfh_f32)   B*N int32
 *   fpfh        out  B*N*33 float32
 *   so3_spfh_f32's outputs are each optional, not both NULL.
 * 1 <= K <= SO3_KNN_MAX_K, 1 <= N <= SO3_ADD_S_MAX_N, B as so3_knn_f32 (B == 0: a no-op).  B, N and K are checked first: B == 0 with
 * a K out of range is an error, B == 0 with NULL pointers is not.
 */
int so3_spfh_f32(const float *X, const float *normals, const int32_t *idx, const int32_t *len, float *spfh, int32_t *pairs, int32_t K,
                 int64_t B, int32_t N, void *stream);
int so3_fpfh_f32(const float *X, const int32_t *idx, const int32_t *len, const float *spfh, const int32_t *pairs, float *fpfh, int32_t K,
                 int64_t B, int32_t N, void *stream);

/* ---- RANSAC over feature matches: global registration from correspondences that are mostly wrong (added in 210) ----
 * The step after FPFH in PCL's SampleConsensusPrerejective and Open3D's registration_ransac_based_on_correspondence: H hypotheses per
 * cloud, each the pose of three sampled pairs, each scored on ALL matched pairs; the best one wins.  Two launches:
 * so3_ransac_score_f32 writes every hypothesis' pose and score, so3_ransac_select_f32 picks the winner and writes what
 * so3_rigid_align_f32 needs to refine it.  Cloud b has n_b = clip(x_len[b], 0, N) source and m_b = clip(y_len[b], 0, M) target points
 * (NULL: all).  The sampler is the caller's: samples (B*H*3) holds indices into the source cloud.
 * VALID PAIR.  Pair i is valid when i < n_b and 0 <= corr[b,i] < m_b (one unsigned compare: -1, M and INT32_MIN are all "no match");
 *   its target is q_i = Q[b, corr[b,i]].  No index addresses anything before it is tested.
 * ADMISSIBLE HYPOTHESIS, a bit definition.  h with (i0, i1, i2) = samples[b,h] is admissible when each i_k lies in [0, N) and names a
 *   valid pair, the three i_k are pairwise distinct, their three corr values are pairwise distinct, and for each edge (a, c) of
 *   (0,1), (0,2), (1,2), with d2(v) = fma(v_z, v_z, fma(v_y, v_y, v_x * v_x)) of rounded coordinate differences,
 *       lp2 = d2(p_a - p_c),  lq2 = d2(q_a - q_c),  s2 = edge_similarity * edge_similarity (one float32 multiply):
 *       lp2 >= s2 * lq2  and  lq2 >= s2 * lp2   (each side one rounded multiply; a NaN fails).
 *   Open3D's edge-length checker on squares; edge_similarity = 0 leaves only the rejection of non-finite edges.
 * POSE.  T_hyp[b,h] is 12 floats, the rows (R | t) of so3_add_s_fwd_f32's pose layout: so3_rigid_align_f32's answer for the three pairs
 *   with unit weights about the pivot (p_i0, q_i0).  An inadmissible hypothesis gets the identity, exactly.  The pose's arithmetic is
 *   NOT part of the bit contract (three pairs give a rank-two H; the rotation's error grows as s1 / s2 of its singular values, and a
 *   collinear triple gets some finite pose and loses the vote); everything below is defined GIVEN the pose that was written.
 * SCORE, a bit definition given T.  r2 = max_distance * max_distance (float32).  For i = 0 .. N-1 ascending, valid pairs only:
 *       x = T p_i, per coordinate fma(T0, p_x, fma(T1, p_y, fma(T2, p_z, T3)));   d2 = d2(x - q_i);
 *       d2 <= r2 (a NaN is no inlier):   count <- count + 1;   err <- err + d2, one float32 chain from +0 in that order.
 *   An inadmissible hypothesis has count = -1, err = 0.
 * SELECTION, a bit definition.  best[b] = the h with the largest count >= 0, among equals the smallest err, among equals the smallest
 *   h; -1 when no hypothesis has count >= 0, and T_best is then the identity.  so3_ransac_select_f32 reads T_hyp, count and err as
 *   given -- it recomputes no pose -- so crafted arrays are legal input.  With T = T_best, for every row i < N:
 *       weights[b,i] = 1 where pair i is valid, best >= 0 and d2 <= r2 (the score's arithmetic), else 0;
 *       targets[b,i] = q_i for a valid pair;  T p_i for an invalid pair with i < n_b (inside the cloud, so that so3_rigid_align_f32's
 *       pivot and "a point of weight 0 must still be finite" hold);  0 for i >= n_b.
 *   inliers[b] = max(count, 0) and rmse[b] = sqrt(err / (float)count) of the winner (IEEE division, correctly rounded root; 0 when
 *   count <= 0);  T_best[b] = the winner's 12 floats.
 * Every element of every output is written.  No atomics, no workspace, no host synchronisation: both calls can be captured in a graph
 * and the same inputs give the same bits.
 *   P  in  B*N*3 float32;  Q  in  B*M*3 float32;  corr  in  B*N int32;  x_len, y_len  in  optional B int32;  samples  in  B*H*3 int32
 *   T_hyp  B*H*12 float32, count  B*H int32, err  B*H float32:   out (so3_ransac_score_f32) / in (so3_ransac_select_f32)
 *   best  out  B int32;  T_best  out  B*12 float32;  inliers  out  B int32;  rmse  out  B float32;  weights  out  B*N float32;
 *   targets  out  B*N*3 float32.  No output is optional.
 * 1 <= N, M <= SO3_ADD_S_MAX_N, 1 <= H <= SO3_RANSAC_MAX_HYPOTHESES, max_distance finite and >= 0, 0 <= edge_similarity <= 1, B as
 * so3_knn_f32.  Checked in this order: B/N/M, H, then B == 0 returns (a no-op), max_distance, edge_similarity, NULL pointers.
 */
#define SO3_RANSAC_MAX_HYPOTHESES 1048576
int so3_ransac_score_f32(const float *P, const float *Q, const int32_t *corr, const int32_t *x_len, const int32_t *y_len,
                         const int32_t *samples, float max_distance, float edge_similarity, float *T_hyp, int32_t *count,
                         float *err, int64_t B, int32_t N, int32_t M, int32_t H, void *stream);
int so3_ransac_select_f32(const float *P, const float *Q, const int32_t *corr, const int32_t *x_len, const int32_t *y_len,
                          const float *T_hyp, const int32_t *count, const float *err, float max_distance, int32_t *best,
                          float *T_best, int32_t *inliers, float *rmse, float *weights, float *targets,
                          int64_t B, int32_t N, int32_t M, int32_t H, void *stream);

/* ---- PointNet++ sampling and grouping: farthest-point sampling and ball query (added in 210) ----
 * The reference's point_cloud/pointnet_utils.py: farthest_point_sample (:53-74, a Python loop of npoint iterations) and
 * query_ball_point (:77-97, a (B,S,N) index tensor sorted along N), each as one launch.
 *
 * THE ARITHMETIC IS A DEFINITION.  Farthest-point sampling is a chain: an argmax that rounds differently changes every later
 * index, and on the reference's own workload the best and the runner-up come within 6e-7 of each other (relative).  So:
 *     d(j, c) = ((dx * dx) + (dy * dy)) + (dz * dz),   dx = x_j - c_x, dy = y_j - c_y, dz = z_j - c_z,
 *   every operation rounded to float32 on its own, no fused multiply-add;
 *     dist_j starts at 1e10f and is updated by   if (d < dist_j) dist_j = d;
 *     the next index is the argmax of dist, the LOWEST index among equal values.
 *   This is index for index what the reference's loop computes in float32 on the CPU from the same start.
 *   Ball membership is   !(d(j, c) > radius * radius)   with the same d and the product rounded to float32.
 *   KNOWN DIFFERENCE from the reference: its query_ball_point takes d from the expanded form |a|^2 + |b|^2 - 2 a.b
 *   (square_distance, :12-31), so a point within rounding of the sphere (| d - r^2 | of the order 1e-6 r^2 .. 1e-5 r^2 for
 *   clouds of unit radius) can fall on the other side.  It is the only difference.
 *   Non-finite coordinates give unspecified indices, but every index stays in [0, N] and the kernels terminate.
 *
 * so3_fps_f32: out[b][0] = start[b];  out[b][i + 1] = the argmax above after the update with centre out[b][i].
 *   xyz      in   B*N*3 float32
 *   start    in   B int32, each in [0, N) (a value outside is clamped into the range)
 *   out      out  B*npoint int32
 *   1 <= N <= SO3_FPS_MAX_N, 1 <= npoint <= SO3_FPS_MAX_N.  npoint > N is legal: once every point has been taken every dist
 *   is 0 and the rule gives index 0.  One workgroup per cloud and all npoint iterations in one launch (the points and their
 *   running minima stay in registers); no atomics, no workspace.
 * so3_ball_query_f32: for centre s of cloud b the first `width` = min(nsample, N) indices j, ascending, of the points inside
 *   the ball; the remaining slots repeat the first hit; a centre WITHOUT a hit gets N in every slot (as the reference does:
 *   an index one past the cloud -- look at count before gathering).
 *   xyz      in   B*N*3 float32;   centres in B*S*3 float32
 *   idx      out  B*S*width int32
 *   count    out  optional B*S int32: the points in the ball, NOT clipped to nsample (asking for it scans the whole cloud;
 *                 without it a centre's scan stops once its row is full)
 *   1 <= N, S <= SO3_ADD_S_MAX_N, 1 <= nsample.  One wave per centre, no atomics, no workspace.
 * Neither call synchronises with the host; both can be captured in a graph and give the same bits from call to call.
 */
#define SO3_FPS_MAX_N 16384
int so3_fps_f32(const float *xyz, const int32_t *start, int32_t *out, int64_t B, int32_t N, int32_t npoint, void *stream);
int so3_ball_query_f32(const float *xyz, const float *centres, float radius, int32_t nsample, int32_t *idx, int32_t *count,
                       int64_t B, int32_t N, int32_t S, void *stream);

/* ---- PointNet++ feature propagation: the three nearest known points and their interpolation (added in 210) ----
 * The non-GEMM half of the reference's PointNetFeaturePropagation.forward (point_cloud/pointnet_utils.py:283-293): a (B,N,S)
 * distance tensor, a full sort along S to keep three columns, five element-wise launches for the weights, a (B,N,3,D) gather,
 * a product and a sum -- here one launch for the search, one for the interpolation and one for its backward.
 *
 * THE ARITHMETIC IS A DEFINITION.
 *   d(n, s) is the d(j, c) of the sampling section above between unknown point n and known point s:
 *       ((dx * dx) + (dy * dy)) + (dz * dz) from coordinate differences, every operation rounded to float32 on its own, no
 *       fused multiply-add.
 *   The neighbours of n are the three smallest under the order "smaller d first, among equal d the LOWER index first",
 *   written in that order.
 *   S < 3 is legal: the min(3, S) real neighbours come first; the remaining slots repeat slot 0's index with dist2 = +inf and
 *   weight 0.
 *   The weights:  r_k = 1.0f / (d_k + 1e-8f)  (r_k = 0 for a padded slot);   w_k = r_k / ((r_0 + r_1) + r_2).
 *       Every addition and every division is an IEEE-754 operation rounded to float32 on its own (the library is built without
 *       fast-math: the divisions are correctly rounded divisions, not reciprocal approximations).  S == 1 gives exactly 1.
 *   The interpolation, in this order:  out = fma(w_2, f_2, fma(w_1, f_1, w_0 * f_0)), f_k = feat[idx_k][c]: one rounded
 *       product and two fused multiply-adds, each rounded once.
 *   The backward:  grad_feat[b][s][c] = sum of w(n,k) * grad_out[b][n][c] over all (n, k) with idx[b][n][k] == s, accumulated
 *       in ASCENDING (n, k) from 0 by  acc = fma(w, g, acc).  The order is part of the definition.
 *   KNOWN DIFFERENCE from the reference: it takes d from the expanded form |a|^2 + |b|^2 - 2 a.b (square_distance, :12-31).
 *   Two known points whose distances to n differ by a few 1e-7 (unit-radius clouds) can swap there, and a true distance of 0 --
 *   every second row where the known points are a subset of the unknown ones, as in the model's fp1 and fp2 -- comes out as
 *   +-1e-7 of cancellation noise, which 1 / (d + 1e-8) turns into arbitrary, even negative, weights.  Here a coincident point
 *   has d == 0 exactly and weight 1 - O(1e-8 / d_1).
 *   A d that overflows float32 and non-finite coordinates give unspecified neighbours and weights, but every index stays in
 *   [0, S) and the kernels terminate.
 *
 * so3_three_nn_f32:
 *   unknown  in   B*N*3 float32;   known in B*S*3 float32
 *   dist2    out  B*N*3 float32: d of the three neighbours, ascending
 *   idx      out  B*N*3 int32
 *   weight   out  optional B*N*3 float32
 *   1 <= N, S <= SO3_ADD_S_MAX_N.  The known cloud goes through on-chip memory in tiles; a launch with few unknown points splits
 *   every point's scan over four waves and merges their lists on (d, idx) -- the result does not depend on the split.
 * so3_three_interpolate_f32 / so3_three_interpolate_bwd_f32: both layouts are contiguous;
 *   channels_first == 0:  feat (B,S,D) -> out (B,N,D);   grad_out (B,N,D) -> grad_feat (B,S,D)   (the reference's internal layout)
 *   channels_first != 0:  feat (B,D,S) -> out (B,D,N);   grad_out (B,D,N) -> grad_feat (B,D,S)   (what the layer receives and
 *                         what its Conv1d takes)
 *   idx      in   B*N*3 int32, each in [0, S).  An index outside is the CALLER'S ERROR; it is clamped into the range by the
 *                 forward and by the backward alike, so it cannot make a kernel touch memory outside the buffers.
 *   weight   in   B*N*3 float32 (any values: the weights need not come from so3_three_nn_f32)
 *   1 <= D <= SO3_THREE_MAX_D.  The backward writes EVERY element of grad_feat (0 for a known point nobody selected); there is
 *   no gradient with respect to weight, idx or the coordinates.
 * None of the three uses atomics, a workspace or a memset, none synchronises with the host; all can be captured in a graph
 * and give the same bits from call to call.  B == 0 is a no-op whatever the pointers.
 */
#define SO3_THREE_MAX_D 65536
int so3_three_nn_f32(const float *unknown, const float *known, float *dist2, int32_t *idx, float *weight, int64_t B, int32_t N,
                     int32_t S, void *stream);
int so3_three_interpolate_f32(const float *feat, const int32_t *idx, const float *weight, float *out, int32_t channels_first,
                              int64_t B, int32_t N, int32_t S, int32_t D, void *stream);
int so3_three_interpolate_bwd_f32(const float *grad_out, const int32_t *idx, const float *weight, float *grad_feat,
                                  int32_t channels_first, int64_t B, int32_t N, int32_t S, int32_t D, void *stream);

/* ---- PointNet++ set abstraction: the grouping gather and its backward (added in 210) ----
 * What every PointNetSetAbstraction / PointNetSetAbstractionMsg forward does between the ball query and its first Conv2d
 * (point_cloud/pointnet_utils.py:117-124 and :234-242): two advanced-index gathers, a subtraction, a cat and a permute that the
 * convolution then makes contiguous -- here one launch that writes the layer's own layout, and one backward call that is a gather.
 *
 *   xyz (B,N,3), centres (B,S,3) and idx (B,S,K) int32 are always in these layouts.  C = 3 + D; D == 0 is legal, and then feat and
 *   grad_feat are not read (pass NULL).
 *   channels_first == 0:  feat (B,N,D);  out / grad_out (B,S,K,C)   (the reference's internal layout)
 *   channels_first != 0:  feat (B,D,N);  out / grad_out (B,C,K,S)   (what the layer receives, and what its permute(0,3,2,1) hands
 *                         to Conv2d)
 *   features_first == 0:  channels 0..2 are the relative coordinates, then the D features   (sample_and_group: cat([xyz_norm, points]))
 *   features_first != 0:  the D features first, then the three relative coordinates   (the Msg layer: cat([grouped_points, grouped_xyz]))
 *
 * THE FORWARD IS A DEFINITION.  A relative coordinate is  xyz[b][idx[b][s][k]][j] - centres[b][s][j],  one float32 subtraction; a
 *   feature is a copy.
 * AN INDEX OUTSIDE [0, N) -- so3_ball_query_f32 writes N into every slot of an empty ball; a negative index falls under the same
 *   rule -- gives 0 IN EVERY CHANNEL of that slot, and the slot takes and gives no gradient: nothing of it reaches grad_xyz, grad_feat
 *   or grad_centres.  No index can make a kernel read or write outside a buffer.  (The reference's index_points raises an IndexError
 *   there.)
 * THE BACKWARD, so3_group_points_bwd_f32:
 *   grad_xyz[b][n][j] and grad_feat[b][n][d] (feat's layout) are the sums of the matching channel of grad_out over all slots (s, k)
 *   with idx[b][s][k] == n;  grad_centres[b][s][j] = 0 - (the sum of coordinate channel j over the valid slots k of row (b, s)).
 *   THE SUMMATION ORDER IS PART OF THE DEFINITION: every sum starts at 0 and takes its terms by plain float32 additions in the
 *   ascending MEMORY order of grad_out's slots --
 *       channels_first == 0:  ascending (s, k), s the slow index;      channels_first != 0:  ascending (k, s), k the slow index;
 *       grad_centres: ascending k in both layouts.
 *   The order does not depend on B, on the launch's grid or on which outputs are requested.
 *   Each of grad_xyz, grad_centres and grad_feat is optional (NULL: not computed).  Every element of a requested output is written
 *   exactly once, 0 for a point nobody selected.  grad_out is read once per 64 points of the cloud (and once more for grad_centres).
 * 1 <= N, S <= SO3_ADD_S_MAX_N, 1 <= K <= SO3_GROUP_MAX_K, 0 <= D <= SO3_THREE_MAX_D.  Offsets into out and grad_out are 64-bit.
 * Neither call uses atomics, a workspace or a memset, neither synchronises with the host; both can be captured in a graph and give
 * the same bits from call to call.  B == 0 is a no-op whatever the pointers.
 */
#define SO3_GROUP_MAX_K 65536
int so3_group_points_f32(const float *xyz, const float *centres, const float *feat, const int32_t *idx, float *out, int32_t features_first,
                         int32_t channels_first, int64_t B, int32_t N, int32_t S, int32_t K, int32_t D, void *stream);
int so3_group_points_bwd_f32(const float *grad_out, const int32_t *idx, float *grad_xyz, float *grad_centres, float *grad_feat,
                             int32_t features_first, int32_t channels_first, int64_t B, int32_t N, int32_t S, int32_t K, int32_t D, void *stream);

/* ---- next row: on-device pair synthesis for Kabsch ------------------------------
 * so3_rotations_axis_angle_f32: the arithmetic of the reference's sampler, point_cloud/prepare.py:21-49
 *   (normalize_vector :12-18, quaternion (cos theta, axis sin theta) -> matrix :27-47), given the random
 *   draws theta (B) and axis (B,3) (the reference draws them with numpy / torch.randn: RNG stays with the caller).
 * so3_kabsch_synth_f32: K5 with the second cloud synthesised on the fly,
 *       q_bi = Rgt_b p_bi + sigma * n(seed, b, i)        (pairing rule point_cloud/main.py:173-181, plus noise)
 *   so only P (12 B per point) is read from HBM instead of P and Q.  n is a stateless counter-based standard
 *   normal (32-bit mix -> three Box-Muller pairs per PAIR of points 64 apart, csrc/so3proj.hip `synth_normal3x2`; restated by the
 *   test oracle, oracle/ `synth_normal_np`).  The stream a seed names belongs to the library's build, not to this
 *   ABI: it is the same on every device and launch shape, and it changed between rounds of this library (last: round 6).
 *   sigma = 0 skips the generator.  R, H as in so3_kabsch_f32.
 */
int so3_rotations_axis_angle_f32(const float *theta, const float *axis, float *R, int64_t B, void *stream);
int so3_kabsch_synth_f32(const float *P, const float *Rgt, float sigma, uint32_t seed, float *R, float *H,
                         int64_t B, int32_t N, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SO3PROJ_H_ */
