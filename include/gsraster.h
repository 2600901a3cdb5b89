/*
 * gsraster.h -- C ABI of libgsraster_hip.so, the MI355X (gfx950) tile rasterizer that
 * replaces GS-LIVM's CudaRasterizer::Rasterizer static API.
 *
 * Every entry point cites the reference interface it replaces (paths relative to the
 * GS-LIVM tree).  All pointers are DEVICE pointers to f32 data unless stated; matrices
 * are 16 floats, column-major (the layout include/gs/cuda_rasterizer/auxiliary.h:48-64
 * indexes).  Nullable pointers follow the reference's convention: NULL == "not
 * provided" (a size-0 tensor in the Torch binding, src/gs/rasterizer.cu:178-193).
 *
 * No Torch, GLM or STL types cross this boundary.  The library never allocates or frees
 * device memory: scratch comes from the three allocator callbacks (forward) or from the
 * blobs those callbacks returned (backward).  All work is enqueued on `stream`
 * (a hipStream_t passed as void*; NULL = the null stream).
 *
 * Errors: functions return a negative gsr_status; gsr_last_error() returns a
 * thread-local message.  (The reference throws std::runtime_error / exits; a C ABI
 * cannot, the binding in gs-livm_amd/csrc/torch_binding.cpp converts.)
 */
#ifndef GSRASTER_H_INCLUDED
#define GSRASTER_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_ABI_VERSION 2

typedef enum gsr_status {
  GSR_OK = 0,
  GSR_ERR_INVALID_ARGUMENT = -1, /* bad shape / null required pointer                 */
  GSR_ERR_ALLOC = -2,            /* an allocator callback returned NULL               */
  GSR_ERR_HIP = -3,              /* a HIP runtime call or kernel launch failed        */
  GSR_ERR_UNSUPPORTED = -4       /* e.g. SH degree > 3, M > 16                        */
} gsr_status;

/* Replaces std::function<char*(size_t)> (include/gs/cuda_rasterizer/rasterizer.h:24-26;
 * Torch side: resizeFunctional, src/gs/rasterize_points.cu:36-44).  Called at most once
 * per gsr_forward per blob; must return device memory (>= `bytes`, 256-B aligned) that
 * stays valid until the matching gsr_backward has completed on the stream. */
typedef char* (*gsr_alloc_fn)(void* ctx, size_t bytes);

/* Alignment of caller tensors (every input and output array of gsr_forward, gsr_backward and gsr_backward_depth):
 * they are contiguous and need only the alignment of their element, 4 bytes -- the library takes its 16-byte copy
 * branches only where the pointer it is handed allows them.  ONE EXCEPTION: `rotations` is read as one 16-byte
 * quaternion per Gaussian and must be 16-byte aligned whenever it is read (no cov3D_precomp).  A misaligned
 * `rotations` is refused with GSR_ERR_INVALID_ARGUMENT before anything is enqueued; the Python and LibTorch hosts
 * pass an aligned copy instead, so their operator surfaces accept any contiguous tensor.
 * The active SH degree D may be below the allocated one: every pair 0 <= D <= 3, (D+1)^2 <= M <= 16 is legal, the
 * coefficients beyond (D+1)^2 are not read and their gradient rows are written as zeros. */

/* Replaces CudaRasterizer::Rasterizer::forward (rasterizer.h:23-51,
 * src/cuda_rasterizer/rasterizer_impl.cu:181-342).
 *   P Gaussians, D = SH degree (0..3), M = SH coefficients per Gaussian (shs is [P][M][3]).
 *   out_color [3][H][W] planar, out_depth [H][W], out_acc [H][W] are fully written.
 *   radii [P] int32 (nullable: an internal array is used, as rasterizer_impl.cu:217-219).
 *   prefiltered / debug: accepted for signature parity; prefiltered has no effect in the
 *   reference forward either; debug != 0 synchronises the
 *   stream after every stage and reports kernel errors (auxiliary.h:146-154).
 * Returns, on success, the BINNING KEY (>= 0): the number to pass to gsr_backward as `R` (and to
 * gsr_binning_view_of) together with the three blobs -- the instance capacity the binning blob was carved for;
 * a negative gsr_status on failure.
 *   - Synchronous forward (a host thread's first forward, every debug != 0 forward, GSR_SYNC_FORWARD=1): the
 *     host waits for num_rendered where the reference has its blocking cudaMemcpy
 *     (rasterizer_impl.cu:277), sizes the binning blob exactly, and the key IS num_rendered.
 *   - Speculative forward (the steady state): the binning blob is allocated for a capacity predicted
 *     from the calling thread's recent forwards (5/4 of the largest of the last four + 64 Ki), every
 *     kernel is enqueued at once and reads num_rendered from device memory, and the host looks at
 *     the count only after the last launch, when it has long been written -- no host wait, no GPU
 *     idle.  The key is the capacity (>= num_rendered).  If num_rendered exceeded the capacity
 *     the binning allocator is called a SECOND time (exact size; the first allocation may be
 *     released) and the binning chain is enqueued again; results are identical either way.
 *   gsr_last_num_rendered() returns the calling thread's last forward's exact num_rendered (the
 *   reference's return value: the instances emitted, sorted and ranged) without touching the device.
 * The host-thread state behind this (mailbox word, counters, prediction) is per thread and device;
 * one thread's forwards must be ordered on the device (ONE stream at a time per host thread -- the
 * reference uses the default stream only); a thread that changes streams is detected and the
 * previous stream is drained first.  Calls from different host threads are independent.
 *
 * Non-finite inputs.  A NaN or +-Inf in a Gaussian is not an error and never leaves a buffer: every index derives from
 * the tile rectangle, which is clamped to the grid after a float -> int conversion that gives 0 for NaN and saturates
 * (v_cvt_i32_f32; the reference's cvt.rzi.s32.f32 does the same).  What the row then does is the reference's own
 * arithmetic, in both binning modes alike (tests/test_gpu_nonfinite.py):
 *   means3D      NaN / +-Inf in any component: the projected centre is NaN or infinite, the rectangle is empty, the row
 *                is culled (radii 0, no gradient).  gsr_mark_visible reports a NaN depth as present (`<=` is false).
 *   scales, rotations, cov3D_precomp
 *                NaN, or an Inf that turns into NaN in the covariance: the radius is NaN -> radii 0, yet the rectangle
 *                of radius 0 is the ONE tile under the centre; the conic is NaN, alpha = min(0.99, NaN) = 0.99: the row
 *                paints that tile.  (The reference leaves this instance's sort key uninitialised; it is emitted here.)
 *                A scale of +Inf is scale-culled.  The row's own gradients are zero (radii 0).
 *   opacities    NaN and +Inf: alpha 0.99 over the whole 3-sigma rectangle.  -Inf: alpha 0.99 where exp(power) has
 *                underflowed to 0 (-Inf * 0 = NaN), nothing elsewhere.  A non-finite opacity is never footprint-culled.
 *                A row that no pixel blended gets exact zero gradients, whatever its opacity.
 *   shs          a NaN colour sum becomes 0 (black): max(NaN, 0) is NaN-ignoring here, where the reference's glm::max
 *                returns NaN.  +Inf gives an infinite colour: infinite / NaN pixels under the row, and NaN gradients
 *                for the rows in front of it on those pixels (the reference's accum_rec recurrence).
 *   colors_precomp  blended as given: non-finite pixels and gradients as for an infinite SH colour.
 * Gradients of rows that share no tile with a poisoned row are unaffected. */
int gsr_forward(gsr_alloc_fn geometry_alloc, void* geometry_ctx, gsr_alloc_fn binning_alloc, void* binning_ctx,
                gsr_alloc_fn image_alloc, void* image_ctx, int P, int D, int M, const float* background, int width,
                int height, const float* means3D, const float* shs, const float* colors_precomp,
                const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                float tan_fovx, float tan_fovy, int prefiltered, float* out_color, float* out_depth, float* out_acc,
                int* radii, int debug, void* stream);

int gsr_last_num_rendered(void);
/* Test / tuning hook for the speculative forward: capacity >= 1 = the calling thread's NEXT forward
 * allocates its binning blob for exactly that many instances (smaller than num_rendered forces the
 * overflow path); 0 = forget the thread's history (its next forward is synchronous); negative = no
 * override.  Returns the previous override (-1 = none). */
long long gsr_set_binning_capacity_hint(long long capacity);
unsigned long long gsr_speculative_forwards(void);  /* process-wide counters */
unsigned long long gsr_speculation_overflows(void);
/* Emit chunks whose chunk-table entries the emitters refused (not a valid descriptor range: the chunk's slots are
 * emitted as tile 0 / Gaussian 0 instead of reading out of bounds).  Zero unless binning has a defect.  Process-wide
 * count of the CURRENT device, never reset; unlike the counters above it reads device memory and so waits for the
 * work already enqueued on the null stream. */
unsigned long long gsr_emit_guard_trips(void);

/* Near/far frames.  A tile's list is depth-ordered and a pixel stops reading it once its transmittance
 * is below 1e-4 (forward.cu:380-383); in dense scenes every tile is finished after a few per cent of
 * its list, and emitting, sorting and ranging the rest is most of the forward.  A speculative forward in
 * the default binning mode whose predicted instance count is at least three times the near budget
 * (GSR_NEAR_ENTRIES list entries per tile, default 320) therefore bins the Gaussians in two chains
 * in depth order: the NEAR Gaussians (until they fill the budget) are binned and blended; then only
 * the FAR Gaussians whose tile rectangle still contains an unfinished tile are binned (whole
 * rectangles) and blended on top.  What is left out lies, in every tile it would have gone to,
 * behind the point where every pixel has stopped: images, n_contrib, final_T and every gradient are
 * bit-identical to the one-chain frame; only the lists (num_rendered, point_list, ranges -- each tile's
 * list is its near segment followed by its far segment, gsr_image_view.ranges / .ranges_far) are
 * shorter.  Frames with gsr_set_reference_rects(1), debug frames and synchronous forwards are never
 * split.  gsr_set_near_far(0) / GSR_NEAR_FAR=0 switches the feature off process-wide; returns the previous value.
 * gsr_set_near_far_thread(mode): the same for the CALLING THREAD's forwards only (1 on, 0 off, negative = follow the
 * process-wide value, the default) -- the reference renders from several threads, and a thread that needs a mode of its
 * own must not disturb the others; returns the thread's previous setting (-1 = none).
 * gsr_last_near_far: 1 if the calling thread's last forward was split, with its two instance counts.
 * gsr_set_near_far_hints (test / tuning hook, calling thread): near list entries per tile (< 0 =
 * default) and the far capacity of the NEXT split forward (< 0 = from history; too small forces the
 * redo path). */
int gsr_set_near_far(int on);
int gsr_set_near_far_thread(int mode);
int gsr_near_far(void);  /* what the calling thread's next forward will use */
int gsr_last_near_far(unsigned* near_instances, unsigned* far_instances);
void gsr_set_near_far_hints(long long near_entries_per_tile, long long far_capacity);
unsigned long long gsr_near_far_forwards(void);
/* Far-chain speculation.  When a thread's last two split forwards left no quad unfinished after the near
 * chain (a dense scene: the far chain's launches found nothing to do), its next split forward is
 *   - asynchronous, where the device supports stream-side waits (hipStreamWaitValue32; GSR_ASYNC_FAR=0
 *     switches this off) and while ONE host thread of the process is rendering (one thread at a time owns the
 *     mechanism, and a process whose rendering hands over between threads twice within 100 ms takes the
 *     host-decided variant below): the far chain is enqueued on a stream of the library's own behind a wait for
 *     the near blend's decision, each of its kernels gated on "needed", and the caller's stream waits
 *     for the frame's go word -- stored by the near blend itself when nothing is left to do, by the far
 *     chain's last kernel otherwise.  gsr_forward returns without waiting for the decision; the far
 *     segment of the binning blob is sized for every instance behind the near budget;
 *   - otherwise decided by the host: the count of unfinished quads arrives in the mailbox where
 *     num_rendered does, and the far chain is enqueued only if it is non-zero (one host round trip).
 * Such a frame also sorts only its NEAR candidates by depth up front (partial depth sort: the Gaussians whose depth key
 * lies in the top-byte groups the near budget can reach); the sort of all P Gaussians moves into the far chain
 * (GSR_FULL_DEPTH_SORT=1: always up front).  gsr_geometry_view.depth_order is the full order only in frames whose far
 * chain ran or that sorted everything up front.
 * Results are identical in every variant.  While an asynchronous frame is in flight,
 * gsr_last_num_rendered / gsr_last_near_far report the near chain's count and add the far chain's once
 * the frame has got there (they never wait).
 * gsr_set_far_speculation (test / tuning hook, calling thread): 1 = the NEXT split forward speculates,
 * 0 = none does, negative = automatic (and the streak restarts); returns the previous setting.
 * gsr_last_far_skipped: 1 if the calling thread's last forward completed without running a far chain. */
int gsr_set_far_speculation(int mode);
int gsr_last_far_skipped(void);
unsigned long long gsr_far_skips(void);       /* process-wide counters */
unsigned long long gsr_far_skip_misses(void);
unsigned long long gsr_async_far_frames(void);
/* Asynchronous frames report their outcome (quads left unfinished, far-chain instances) through a mailbox slot of
 * their own; up to eight such frames of a thread may be outstanding.  gsr_async_outcomes_pending: how many of the calling
 * thread's are still unresolved (never waits); gsr_async_outcomes_lost: frames whose slot had to be reused before it
 * was read (a ninth frame in flight) -- each is counted as a miss by the speculation rule.  Process-wide counter. */
int gsr_async_outcomes_pending(void);
unsigned long long gsr_async_outcomes_lost(void);
/* What gsr_backward knows about the forward that filled an image blob (tile order already computed, frame was split)
 * is kept per blob address for as long as the blob may be differentiated; a backward that finds nothing (more than
 * 4096 blobs alive) takes the general path -- same results, one or two launches more -- and is counted here. */
unsigned long long gsr_frame_note_misses(void);
/* Per-view histories.  Everything a speculative forward predicts from -- the binning capacity, the far capacity, the
 * far-chain speculation's streak, the near budget below -- is kept per VIEW of the calling thread: a view is recognised
 * by the device address of its view matrix and the image size (the reference renders several keyframes in turn before
 * one backward, each Camera holding its matrices for its lifetime: lioOptimization.cpp:1691-1737, camera.cu:36-48).
 * Up to 32 views per thread, least recently used replaced; a view seen for the first time starts from the thread's most
 * recently used history, so a caller with one camera, or one that passes a fresh matrix tensor every frame, sees the
 * per-thread behaviour.  A wrong guess costs a redo or a far chain, never a result.
 * Adaptive near budget (per view).  The budget of a split frame is GSR_NEAR_ENTRIES (320) list entries per tile
 * times scale / 256.  A frame whose far chain ran, over less than four times the near chain's instances, raises the
 * scale by 64 (a quarter of the configured budget), up to 768, ON PROBATION: if the view's next frame still leaves more
 * than three quarters of those quads unfinished, the tiles do not finish for lack of budget (sky, the border of the
 * map) -- the raise is taken back and none is tried for 256 frames of the view.  Sixty-four frames in a row without a
 * far chain lower the scale by 16, down to 256.  gsr_near_budget_scale returns the current scale of the view of the
 * calling thread's last forward; gsr_near_budget_feedback (test hook) feeds the outcome of a frame -- unfinished quads
 * after the near chain, near and far instance counts -- to that view's rule as a forward does and returns the scale
 * after it.  The rule rests while gsr_set_near_far_hints sets the budget. */
unsigned gsr_near_budget_scale(void);
unsigned gsr_near_budget_feedback(unsigned unfinished_quads, unsigned near_instances, unsigned far_instances);
/* Eight misses in a row of frames that splitting does not shorten by a quarter (near + far instances against all the
 * frame's; or a far chain of at least four times the near chain: a sparse scene) pause the splitting: the view's next
 * 256 frames are binned in one chain, then it tries again.  gsr_near_far_pause(frames): returns the frames left of the
 * pause of the view of the calling thread's last forward and, if frames >= 0, sets them (0 ends a pause). */
int gsr_near_far_pause(int frames);

/* Replaces CudaRasterizer::Rasterizer::backward (rasterizer.h:53-88,
 * rasterizer_impl.cu:346-457).  geom/binning/image blobs are the ones the forward
 * allocator callbacks returned; R is gsr_forward's return value (the binning key).
 * The nine gradient outputs are FULLY OVERWRITTEN (Gaussians with radii <= 0 get
 * zeros), so the caller need not pre-zero them (the reference requires zeroed buffers,
 * rasterize_points.cu:173-181; zeroed buffers remain valid input).
 *   dL_dmean2D [P][3] (.x,.y written, .z = 0), dL_dconic [P][4] (.x,.y,.w; .z = 0),
 *   dL_dopacity [P], dL_dcolor [P][3], dL_dmean3D [P][3], dL_dcov3D [P][6],
 *   (dL_dcov3D may be NULL when cov3D_precomp is NULL: the gradient w.r.t. a covariance the library computed
 *   itself from scales and rotations is an intermediate; it is then not written),
 *   dL_dsh [P][M][3], dL_dscale [P][3], dL_drot [P][4].
 * The gradient w.r.t. depth is not an input, exactly as in the reference
 * (src/gs/rasterizer.cu:79; backward.cu:451-452). */
int gsr_backward(int P, int D, int M, int R, const float* background, int width, int height, const float* means3D,
                 const float* shs, const float* colors_precomp, const float* scales, float scale_modifier,
                 const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                 const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy, const int* radii,
                 char* geom_buffer, char* binning_buffer, char* image_buffer, const float* dL_dpix,
                 const float* dL_dacc, float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor,
                 float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot, int debug,
                 void* stream);

/* gsr_backward with a gradient w.r.t. the rendered depth (out_depth = sum_i z_i alpha_i T_i, z the view-space depth):
 * an extension, the reference has no such path.  Same arguments, same validation and same nine outputs as
 * gsr_backward, plus
 *   dL_ddepth  [H][W]  in:  dL/d out_depth,
 *   dL_ddepths [P]     out: dL/dz_i = sum over the pixels that take the Gaussian of alpha T dL_ddepth; an intermediate
 *                           like dL_dconic, fully overwritten (0 for radii <= 0 and for Gaussians no pixel took).
 * dL_ddepth reaches alpha (z_i dL_ddepth joins colour . dL_dpix + dL_dacc of every splat) and, through dL_ddepths and the
 * third row of the view matrix, dL_dmean3D.  A null dL_ddepth or dL_ddepths is GSR_ERR_INVALID_ARGUMENT (nothing is
 * launched or written).  With dL_ddepth all zero the nine outputs are bit-equal to gsr_backward's.  Either entry point
 * leaves the blobs ready for the other. */
int gsr_backward_depth(int P, int D, int M, int R, const float* background, int width, int height,
                       const float* means3D, const float* shs, const float* colors_precomp, const float* scales,
                       float scale_modifier, const float* rotations, const float* cov3D_precomp,
                       const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                       float tan_fovy, const int* radii, char* geom_buffer, char* binning_buffer, char* image_buffer,
                       const float* dL_dpix, const float* dL_dacc, const float* dL_ddepth, float* dL_dmean2D,
                       float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D,
                       float* dL_dsh, float* dL_dscale, float* dL_drot, float* dL_ddepths, int debug, void* stream);

/* The camera pose gradient (an extension, the reference's poses are constants): six numbers from what gsr_backward or
 * gsr_backward_depth was given and wrote.  Call it after either, on the same stream, with the same inputs and that
 * call's dL_dmean2D, dL_dconic, dL_dmean3D and (after gsr_backward_depth; else NULL) dL_ddepths.
 *
 * Convention.  The pose is the world-to-camera transform T_cw = [R | T]; the view matrix is its transpose in memory
 * (column-major: R[r][k] = viewmatrix[r + 4k], t = R p + (viewmatrix[12], [13], [14])).  The tangent is a LEFT
 * perturbation in the camera frame, T_cw(xi) = Exp(xi^) T_cw with xi = (rho, phi): rho the translation part, phi the
 * rotation part, both in camera axes.  dL_dpose[6] = dL/dxi at xi = 0, [0:3] = rho, [3:6] = phi, where viewmatrix(xi)
 * is the transpose of T_cw(xi), projmatrix(xi) = viewmatrix(xi) . P with the caller's pose-independent projection P,
 * and campos(xi) = -R(xi)^T T(xi).  The visible set, the tile lists, the SH clamp flags and the per-pixel cuts are held
 * fixed and the backward's departures from the exact derivative apply unchanged: it is the gradient gsr_backward would
 * hand out were the camera one of its leaves:
 *   dL/drho = R sum_i dL_dmean3D_i
 *   dL/dphi = sum_i t_i x (R dm_geo,i) + 2 sum_i axial(G_cam,i Sigma_cam,i - Sigma_cam,i G_cam,i)
 * (dm_geo: dL_dmean3D without its SH view-direction part, which a rotation about the camera centre leaves alone; G the
 * symmetric form of dL_dcov3D; X_cam = R X R^T; axial(A) = (A[2][1], A[0][2], A[1][0])).  dm_geo and G are recomputed
 * with the backward's own arithmetic, the same bits; no SH coefficient is read and dL_dcov3D is not needed.
 *
 * Rows with radii <= 0 contribute nothing and nothing but their radius is read: their gradient rows may hold anything.
 * The per-row terms are float32, widened to float64 and summed in a fixed order that depends on P alone (no atomics):
 * the result is bitwise reproducible from run to run and from machine to machine.  A non-finite value in a visible
 * row makes the affected components non-finite.  P == 0 writes six zeros.
 *
 * No host wait, no allocation: two launches on `stream`.  `workspace` holds gsr_pose_gradient_workspace(P) bytes
 * (0 only for P < 0) and needs no alignment (the size includes the slack).  GSR_ERR_INVALID_ARGUMENT, before anything
 * is enqueued or written, for: P < 0, a non-positive width / height, a non-finite or non-positive tan_fov, a null
 * dL_dpose / workspace / required input, scales without rotations (or the reverse), either of them together with
 * cov3D_precomp or none of the three, rotations not 16-byte aligned, workspace_bytes below the query (the message
 * names the bytes needed). */
size_t gsr_pose_gradient_workspace(int P);
int gsr_pose_gradient(int P, int width, int height, const float* means3D, const float* scales, float scale_modifier,
                      const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                      const float* projmatrix, float tan_fovx, float tan_fovy, const int* radii,
                      const float* dL_dmean2D, const float* dL_dconic, const float* dL_ddepths /* nullable */,
                      const float* dL_dmean3D, float* dL_dpose /* [6] */, char* workspace, size_t workspace_bytes,
                      void* stream);

/* Replaces CudaRasterizer::Rasterizer::markVisible (rasterizer.h:21,
 * rasterizer_impl.cu:128-135): present[i] = z_view > 0.2 (1-byte bool). */
int gsr_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     unsigned char* present, void* stream);

/* Replace required<GeometryState|ImageState|BinningState>() (rasterizer_impl.h:62-67):
 * bytes the corresponding allocator callback will be asked for. */
size_t gsr_geometry_bytes(int P);
size_t gsr_image_bytes(int width, int height);
size_t gsr_binning_bytes(int R);

/* Views into the opaque blobs, for parity tests and tooling (the reference exposes the
 * same arrays through GeometryState/BinningState/ImageState, rasterizer_impl.h:28-60).
 * Pointers are device pointers into the blob; arrays the implementation does not keep
 * are NULL. */
typedef struct gsr_geometry_view {
  const float* depths;            /* NULL: not kept (the view-space depth is splats[i][9])              */
  const int32_t* radii;           /* [P] internal radii: valid only when gsr_forward got radii == NULL  */
  const float* splats;            /* [P][12]: x, y, conic.x, conic.y, conic.z, opacity, r, g, b, depth, hx, hy */
  const float* cov3D;             /* [P][6] filled only when the forward ran with debug != 0 (the backward
                                     recomputes the covariance from scale and rotation)                 */
  const uint32_t* tiles_touched;  /* NULL: not kept separately (gpack[i][0])                            */
  const uint32_t* point_offsets;  /* [P] inclusive scan in id order (the reference's array; unused by this
                                     pipeline: filled only when the forward ran with debug != 0) */
  const uint8_t* clamped;         /* [P] bit0..2 = r,g,b clamp flags      */
  const uint32_t* depth_order;    /* [P] Gaussian ids by (depth bits, id); culled Gaussians last */
  const uint32_t* num_rendered;   /* device counters of the forward: [0] instances of all Gaussians (= num_rendered of a
                                     one-chain frame); near/far frames ([12] == 1): [6] near instances, [8] far
                                     instances (num_rendered = [6] + [8]), [7] first far Gaussian in depth_order,
                                     [9] tiles unfinished after the near phase, [10] far Gaussians emitted */
  const uint32_t* gpack;          /* [P][2]: tiles touched, packed tile rect x0 | y0 << 10 | width << 20 */
} gsr_geometry_view;
/* The reference's 64-bit sorted key of instance i is ((uint64)tile << 32) | bits(depths[point_list[i]]) with
 * tile = the tile whose range [ranges[tile][0], ranges[tile][1]) contains i: this implementation sorts the
 * Gaussians by depth once and the instances by a 16- or 32-bit tile id only (gs-livm_amd/csrc/radix_sort.hip);
 * the sorted tile ids are scratch (overwritten by the backward), so the view exposes point_list and the keys
 * are implied by ranges + point_list. */
typedef struct gsr_binning_view {
  const uint32_t* point_list;     /* [R] sorted Gaussian ids              */
} gsr_binning_view;
typedef struct gsr_image_view {
  const uint32_t* ranges;         /* [tiles][2] the tile's list segment in point_list (near segment of a near/far frame) */
  const float* final_T;           /* [H][W]                               */
  const uint32_t* n_contrib;      /* [H][W]                               */
  const uint32_t* quad_last;      /* [tiles][4] max n_contrib inside each 8x8 quad of the tile (0,1 = top, 2,3 = bottom);
                                     the tile's maximum = list entries the backward walks */
  const uint32_t* ranges_far;     /* [tiles][2] near/far frames: the far segment that follows `ranges` in the tile's
                                     list (positions count through both); (0, 0) otherwise */
} gsr_image_view;
int gsr_geometry_view_of(char* geom_buffer, int P, gsr_geometry_view* out);
int gsr_binning_view_of(char* binning_buffer, int R, gsr_binning_view* out);
int gsr_image_view_of(char* image_buffer, int width, int height, gsr_image_view* out);

/* Binning mode.  The reference emits one (Gaussian, tile) instance for EVERY tile of the square
 * getRect() puts around the 3-sigma radius (include/gs/cuda_rasterizer/auxiliary.h:39-46,
 * duplicateWithKeys, src/cuda_rasterizer/rasterizer_impl.cu:64-101) and then skips, pixel by pixel, the
 * instances whose alpha stays below 1/255 (forward.cu:374-376).
 *   0 (default): "culled" -- an instance is emitted only where the Gaussian's exact-conservative
 *      alpha >= 1/255 footprint box overlaps the tile.  Images, radii and gradients are unchanged;
 *      tiles_touched, num_rendered, the per-tile lists, ranges and n_contrib describe the shorter lists.
 *   1: "reference" -- getRect's square as it is: tiles_touched, num_rendered, point_list, ranges and
 *      n_contrib equal the reference's bit for bit (about 1.4x the instances at 2 M Gaussians, 1080p).
 * Process-wide default, read at every gsr_forward (a backward follows the mode its forward ran in: the rectangles
 * are stored in the blobs); the initial value comes from the environment variable GSR_REFERENCE_RECTS
 * (unset / "0" = culled).  gsr_set_reference_rects returns the previous value.
 * gsr_set_reference_rects_thread(mode): the mode of the CALLING THREAD's forwards only (1 / 0; negative = follow the
 * process-wide value, the default); returns the thread's previous setting (-1 = none).  gsr_reference_rects: what the
 * calling thread's next forward will use. */
int gsr_set_reference_rects(int on);
int gsr_set_reference_rects_thread(int mode);
int gsr_reference_rects(void);

/* getHigherMsb (rasterizer_impl.cu:35-48): number of tile-id bits the sort covers. */
uint32_t gsr_higher_msb(uint32_t n);

/* ---- "next" row: the caller's per-Gaussian elementwise work, fused ----
 * gsr_activate replaces the five Torch ops of GaussianModel's getters (include/gs/gs/gaussian.cuh:40-54):
 *   scales = exp(_scaling) [P][3], rotations = normalize(_rotation) [P][4] (x / max(|x|, 1e-12)),
 *   opacities = sigmoid(_opacity) [P], shs = cat(_features_dc [P][1][3], _features_rest [P][M-1][3], 1).
 * gsr_activate_backward is the matching chain rule (needs the raw rotation and the activated scales /
 * opacities); every output element is written.
 * gsr_adam_step is torch::optim::Adam::step (as configured in src/gs/gaussian.cu:396-428: per-group lr,
 * no weight decay, no amsgrad) for up to 8 tensors in ONE launch; `step` counts from 1; zero_grads != 0
 * clears the gradients it consumed (the reference's zero_grad, src/liw/lioOptimization.cpp:1831-1832).
 * beta1 / beta2 / eps are doubles as in torch::optim::AdamOptions: 1 - beta is formed in double and then narrowed.
 * Pointer arrays are HOST arrays of device pointers. */
int gsr_activate(int P, int M, const float* scaling_raw, const float* rotation_raw, const float* opacity_raw,
                 const float* features_dc, const float* features_rest, float* scales, float* rotations,
                 float* opacities, float* shs, void* stream);
int gsr_activate_backward(int P, int M, const float* rotation_raw, const float* scales, const float* opacities,
                          const float* dL_dscales, const float* dL_drotations, const float* dL_dopacities,
                          const float* dL_dshs, float* dL_dscaling_raw, float* dL_drotation_raw,
                          float* dL_dopacity_raw, float* dL_dfeatures_dc, float* dL_dfeatures_rest, void* stream);
/* gsr_model_step: the whole optimiser tail in one pass over the model -- gsr_activate_backward's chain rule, Adam on
 * the six groups (order xyz, features_dc, features_rest, scaling, rotation, opacity: the reference's group order,
 * src/gs/gaussian.cu:396-428) and gsr_activate of the UPDATED parameters for the next forward (outputs nullable).
 * Gradients are w.r.t. xyz and the ACTIVATED scales / rotations / opacities / shs, i.e. exactly what the
 * rasterizer's backward returns; the raw-space gradients never reach memory.  Same arithmetic as the three
 * separate entry points. */
int gsr_model_step(int P, int M, float* const* params6, float* const* exp_avg6, float* const* exp_avg_sq6,
                   const float* dL_dxyz, const float* dL_dscales, const float* dL_drotations, const float* dL_dopacities,
                   const float* dL_dshs, float* scales_out, float* rotations_out, float* opacities_out, float* shs_out,
                   const float* lr6, double beta1, double beta2, double eps, int step, void* stream);
int gsr_adam_step(int n_tensors, float* const* params, float* const* grads, float* const* exp_avg,
                  float* const* exp_avg_sq, const size_t* numel, const float* lr, double beta1, double beta2, double eps,
                  int step, int zero_grads, void* stream);

/* ---- "next" row: the photometric loss that follows every render, fused ----
 *   L = (1 - lambda) * mean|img - gt| + lambda * (1 - mean(SSIM(img, gt)))
 * replaces gaussian_splatting::l1_loss + ::ssim (include/gs/gs/loss_utils.cuh:11-13,43-70; combined at
 * src/liw/lioOptimization.cpp:1705-1710) and their autograd: five grouped 11x11 conv2d per view there, three
 * launches here.  img/gt: [channels][H][W] device f32; window11_host: the 11 taps of the separable window on the
 * HOST (the reference's 2-D window is their outer product, loss_utils.cuh:33-37; it need not be symmetric);
 * zero padding 5 like conv2d(padding = window_size/2).  loss_out3 (device) = {L, mean L1, mean SSIM};
 * dL_dimg (nullable) = dL/dimg for upstream gradient 1.  Deterministic (fixed-order reductions). */
size_t gsr_photometric_loss_workspace(int channels, int height, int width);
int gsr_photometric_loss(int channels, int height, int width, const float* img, const float* gt,
                         const float* window11_host, float lambda_dssim, float* loss_out3, float* dL_dimg,
                         char* workspace, size_t workspace_bytes, void* stream);

/* ---- per-keyframe exposure compensation, fused into the photometric loss (an extension: the reference has no such
 * term; csrc/exposure.hip) ----
 *   x'(p) = fma(g_c, x(p), b_c),   L = (1 - lambda) * mean|x' - gt| + lambda * (1 - mean(SSIM(x', gt)))
 * for keyframes of auto-exposure / auto-gain cameras: the brightness step between keyframes goes to 2 C numbers per
 * keyframe instead of the SH coefficients, the opacities and the pose.  exposure: [channels][2] device f32,
 * exposure[c] = (g_c, b_c); the identity is (1, 0).  The gain enters linearly -- a log-gain g = exp(a) is the host's,
 * on C numbers.  Everything else is gsr_photometric_loss's, taken on x': img / gt / window11_host / loss_out3 as
 * there, zero padding of the COMPENSATED image (outside the image x' is 0, not b_c).
 * With G = dL/dx' for upstream gradient 1:
 *   dL_dimg[c][p] = g_c G(p)        dL_dexposure[c] = (sum_p G(p) x(p), sum_p G(p))  -- x the ORIGINAL image --
 * dL_dexposure: [channels][2] device f32.  dL_dimg and dL_dexposure are both given (three launches) or both null (two
 * launches, no gradient); one without the other is refused.  Refusals, in this order: a non-positive dimension, a
 * plane of 2^31 - 1 pixels or more, a null img / gt / exposure / window11_host / loss_out3 / workspace, one gradient
 * pointer without the other, workspace_bytes below gsr_exposure_loss_workspace (which returns 0 for a refused shape);
 * nothing is launched or written then.  The workspace may sit at any 4-byte aligned address.
 * No host wait, no allocation, the caller's stream.  Deterministic: the two exposure sums are float64, added per work
 * unit and then per channel in a fixed order, no atomics, narrowed once.  At exposure = identity and an img without
 * negative zeros every output equals gsr_photometric_loss's bit for bit.
 * gsr_apply_exposure: out[c][p] = fma(g_c, img[c][p], b_c), one launch (evaluation and export).  img / out:
 * [channels][H][W] device f32 at any 4-byte aligned address; out == img is allowed, any other overlap is not. */
size_t gsr_exposure_loss_workspace(int channels, int height, int width);
int gsr_exposure_loss(int channels, int height, int width, const float* img, const float* gt,
                      const float* exposure /* device [channels][2] */, const float* window11_host,
                      float lambda_dssim, float* loss_out3, float* dL_dimg, float* dL_dexposure,
                      char* workspace, size_t workspace_bytes, void* stream);
int gsr_apply_exposure(int channels, int height, int width, const float* img, const float* exposure,
                       float* out, void* stream);

/* ---- the weighted photometric loss: per-pixel weights, a silhouette gate and the exposure, each optional (an
 * extension: the reference has no such term; csrc/weighted.hip) ----
 *   x'(p) = fma(g_c, x(p), b_c) with an exposure, x(p) without one
 *   w(p)  = weights(p) * [acc(p) >= acc_min]          (absent weights: 1; absent acc: no gate; a NaN acc: weight 0)
 *   S     = sum_p w(p)    over the H W pixels: weights and acc are [H][W] device f32, shared by the channels
 *   l1    = sum_c sum_p w |x' - gt| / (C S)           ssim = sum_c sum_q w(q) SSIM_c(q) / (C S)
 *   L     = (1 - lambda) l1 + lambda (1 - ssim)       mse_c = sum_p w (x' - gt)^2 / S
 * SSIM_c is gsr_photometric_loss's, its windows over the FULL x' and gt (zero padding of the compensated image): the
 * weights select where the loss is taken, not what the windows see.  For undistortion borders, sky and dynamic-object
 * masks, texture weights and tracking over the mapped pixels only (acc = the render's silhouette).
 * out6 (device) = {L, l1, ssim, S, mean_c mse_c, psnr}, psnr = gsr_image_metrics's rule on mse_c (+inf where mse_c = 0).
 * With G = dL/dx' for upstream gradient 1:  dL_dimg[c][p] = g_c G(p) (G without an exposure),
 * dL_dexposure[c] = (sum_p G x, sum_p G), x the ORIGINAL image.  Weights and acc get no gradient: the gate is a step.
 * dL_dimg is nullable; dL_dexposure exists only with an exposure, and then both gradients are given or both null.
 * Launches: forward and finish, and with a gradient the backward between them (three in all, as gsr_exposure_loss):
 * 1 / (C S) is formed on the device by every workgroup of the backward, in one fixed order.  No host wait, no
 * allocation, the caller's stream; deterministic (fixed-order reductions, no atomics).  The S of out6[3] and the S behind
 * every gradient element are the same bits.
 * S = 0 (nothing supervised): L = l1 = ssim = mse = 0, psnr = +inf, every gradient element zero, nothing non-finite.
 * Weights are the caller's contract: finite and >= 0.  A ZERO WEIGHT DOES NOT PROTECT AGAINST A NON-FINITE PIXEL of
 * img or gt: the SSIM windows of the weighted pixels within 5 pixels of it read it.
 * With weights absent or all one and no gate, {L, l1, ssim}, dL_dimg and dL_dexposure equal gsr_exposure_loss's bit for
 * bit (gsr_photometric_loss's without an exposure); weights scaled by a power of two change S and nothing else.
 * Refusals, in this order: a non-positive dimension, a plane of 2^31 - 1 pixels or more, a null img / gt /
 * window11_host / out6 / workspace, dL_dexposure without exposure, exposure with only one of dL_dimg and dL_dexposure,
 * a non-finite acc_min with acc given, workspace_bytes below gsr_weighted_loss_workspace (which returns 0 for a refused
 * shape); nothing is launched or written then.  The workspace may sit at any 4-byte aligned address. */
size_t gsr_weighted_loss_workspace(int channels, int height, int width);
int gsr_weighted_loss(int channels, int height, int width, const float* img, const float* gt,
                      const float* weights /* device [H][W], nullable */, const float* acc /* device [H][W], nullable */,
                      float acc_min, const float* exposure /* device [channels][2], nullable */,
                      const float* window11_host, float lambda_dssim, float* out6, float* dL_dimg,
                      float* dL_dexposure, char* workspace, size_t workspace_bytes, void* stream);

/* ---- the LiDAR similarity loss (step 3 of optimize_vis), fused ----
 *   r = mean(scaling[sel]) (one scalar over the 3n selected elements),  d_ij = |points_i - xyz[sel_j]|,
 *   L = lambda * mean_i min_j max(d_ij - r, 0) = lambda / m * sum_i max(min_j d_ij - r, 0)
 * replaces GaussianModel::compute_min_distance (src/gs/gaussian.cu:87-114) as calcSimiLoss calls it (:201-239; call
 * site src/liw/lioOptimization.cpp:1675, lambda_depth_simi of config/basic_common.yaml:64) and its autograd: the
 * [m,n,3] expansions there, a nearest-neighbour search and one clamp per point here, in three launches.
 * points [m,3] device f32: the LiDAR points that are left after selection and subsampling (the cap of MAX_SIMI = 500,
 * include/gs/gp3d/gp_types.h:15, is the host's policy; m and n are bounded by int only).  sel [n] device int32: the
 * rows of the selected voxels' Gaussians, ascending, unique, each < P (what loss_mask.nonzero() yields, :219-221).
 * xyz [P,3]: the model's _xyz; scaling [P,3]: the ACTIVATED scales (Get_scaling()).
 * out3 (device) = {L, mean clamped distance (L before lambda), r}.
 * grad_xyz / grad_scaling (nullable, [P,3]) = dL/dxyz, dL/dscaling for upstream gradient 1: with accumulate = 0 the
 * selected rows are WRITTEN and every other row is left untouched (the caller owns zero-filling), with accumulate = 1
 * the selected rows are ADDED TO, so that the term lands in the buffers the rasterizer's backward already filled.
 * A point with min_j d_ij <= r contributes nothing; of two centres at bit-equal distance the earlier in sel is taken
 * (the reference leaves both cases to Torch's tie rules).  m == 0 or n == 0: returns 0 with out3 = {0, 0, 0}.
 * Deterministic (no float atomics, fixed-order reductions), no host synchronisation; workspace sized by the query. */
size_t gsr_similarity_loss_workspace(int m, int n);
int gsr_similarity_loss(int P, int m, int n, const float* points, const int* sel, const float* xyz,
                        const float* scaling, float lambda, float* out3, float* grad_xyz, float* grad_scaling,
                        int accumulate, char* workspace, size_t workspace_bytes, void* stream);

/* ---- the point-to-plane LiDAR loss on oriented surfels (an extension: the reference has no such term), fused ----
 * The similarity loss above never reads the rotation; this term holds a surfel's thinnest axis to the points near it.
 * points [m,3], sel [n] (ascending unique rows < P), xyz [P,3]: as gsr_similarity_loss takes them; scaling [P,3] and
 * rotation [P,4] are the ACTIVATED values, the quaternion (w, x, y, z) used as given and NOT renormalised, as the
 * rasterizer uses it.  R(q) =
 *   [[1-2(y^2+z^2), 2(xy-wz), 2(xz+wy)], [2(xy+wz), 1-2(x^2+z^2), 2(yz-wx)], [2(xz-wy), 2(yz+wx), 1-2(x^2+y^2)]]
 * and its column k is the axis that belongs to scaling[.][k] (Sigma = R S^2 R^T).
 * Per selected row j: k*_j = index of the smallest of its three scales (strict < from index 0: the lowest index wins
 * a tie), n_j = column k*_j of R(q_j).
 * Per point i: j(i) = the nearest selected centre by the similarity loss's rule (the same FMA chain, strict comparison,
 * the lower position in sel on a bit-equal tie), v_i = p_i - xyz_j, d_i = |v_i|, g_i = [d_i <= max_dist], e_i = n_j . v_i,
 *   rho(e)  = |e| for huber = 0;  e^2 / (2 huber) where |e| <= huber, |e| - huber / 2 beyond it, for huber > 0
 *   rho'(e) = sign(e) with sign(0) = 0;  e / huber inside the knee
 *   L_plane = lambda / m * sum_i g_i rho(e_i)  (normalised by all m points),  L_flat = lambda_flat / n * sum_j scaling[j][k*_j]
 * out4 (device) = {L_plane + L_flat, sum_i g_i rho(e_i) / m, sum_j scaling[j][k*_j] / n, sum_i g_i / m}.
 * grad_xyz [P,3], grad_scaling [P,3], grad_rotation [P,4] (each nullable) for upstream gradient 1, with
 * A_j = sum_{i -> j} g_i rho'(e_i) and B_j = sum_{i -> j} g_i rho'(e_i) v_i:
 *   grad_xyz[j] = -(lambda / m) A_j n_j;  grad_rotation[j] = (dn_j/dq)^T (lambda / m) B_j, the 3x4 Jacobian of the column
 *   of the polynomial above, w included, with no normalisation term (the activation's backward owns that);
 *   grad_scaling[j][k*_j] = lambda_flat / n and 0 in the other two elements (the choice of k* carries no gradient).
 * accumulate = 0 / 1 as gsr_similarity_loss: selected rows are WRITTEN or ADDED TO, every other row is untouched.
 * A non-finite point or centre that wins no comparison contributes 0 and writes nothing.  m == 0 or n == 0: returns 0
 * with out4 = {0, 0, 0, 0}, no gradient.
 * Refused (GSR_ERR_INVALID_ARGUMENT, nothing launched or written), in this order: negative P, m or n; n > P; n beyond
 * gsr_similarity_loss's bound; lambda, huber or lambda_flat not finite or negative; max_dist NaN or <= 0 (+inf is
 * allowed: no gate); a null out4; with m, n > 0 a null points / sel / xyz / scaling / rotation / workspace;
 * workspace_bytes below the query (which returns 0 for a refused or empty shape); a float or int array off 4-byte
 * alignment.  The workspace itself needs no alignment.
 * Deterministic (no float atomics, fixed-order reductions), three launches on the caller's stream, no host
 * synchronisation, no allocation.  Profiled under k_simi_nearest / k_simi_points / k_simi_grads (the id word is full). */
size_t gsr_surfel_plane_loss_workspace(int m, int n);
int gsr_surfel_plane_loss(int P, int m, int n, const float* points, const int* sel, const float* xyz,
                          const float* scaling, const float* rotation, float lambda, float huber, float max_dist,
                          float lambda_flat, float* out4, float* grad_xyz, float* grad_scaling, float* grad_rotation,
                          int accumulate, char* workspace, size_t workspace_bytes, void* stream);

/* ---- rendered normal maps and the depth-normal consistency loss (an extension: the reference has neither) ----
 * gsr_blend_attributes: a forward-only pass behind a completed gsr_forward, in gsr_contribution's shape (P, R, width,
 * height and the three state blobs as that call takes them).  attributes [P][channels] float32, channels 1..4;
 * out [channels][height][width] planar float32:
 *   out[c][pixel] = sum over the splats the pixel took, front to back, of attributes[splat][c] * alpha * T
 * with the forward's own alpha and T and its take rule (gsr_contribution), accumulated by fused multiply-adds in list
 * order as the forward accumulates colour and depth: attributes = 1 gives the forward's acc image bit for bit, the
 * splats' view depths its depth image, the colours (under a zero background) its colour image.  There is no background
 * term.  EVERY element of out is written; a pixel that takes nothing reads +0.0.  Rows the forward culled are never
 * read.  P == 0 or R == 0: legal, out is zeros written by a fill and the blobs are not read.  One launch, plain stores,
 * no atomics: bitwise reproducible.  Profiled under k_visibility.
 * Refused, in this order: channels outside 1..4; a negative P or R, a non-positive width or height; width * height
 * >= 2^31; a null out, and with P, R > 0 null attributes or a null blob; attributes or out off 4-byte alignment.
 *
 * gsr_surfel_normals: one launch, one thread per row.  xyz [P,3], scaling [P,3] and rotation [P,4] are the ACTIVATED
 * values as gsr_surfel_plane_loss takes them; T_cw12 is [R | t] on the HOST, row-major 3 x 4, x_c = R x_w + t.
 *   k* and n_w = column k* of R(q): as gsr_surfel_plane_loss (lowest index on a tie, q not renormalised)
 *   n_c = R n_w, p_c = R x + t, normals[i] = n_c, negated when n_c . p_c > 0 (exactly 0: not negated)
 * normals [P,3]: every row is written, whatever the rasterizer's radii.  Explicit fused multiply-adds throughout.
 * Refused, in this order: negative P; with P > 0 a null pointer; an array off 4-byte alignment.  Profiled under
 * k_visibility.
 *
 * gsr_normal_consistency_loss: depth D and acc A are the rasterizer's second and third outputs [H][W], normals N is
 * [3][H][W] = sum n_c alpha T (gsr_blend_attributes of gsr_surfel_normals), un-normalised.  fx, fy, cx, cy: the pinhole
 * under which pixel (u, v) of a render is pixel (u, v) (cx = (W - 1) / 2 for a centred camera).  At pixel (u, v):
 *   z = D / A,  X = ((u - cx) z / fx, (v - cy) z / fy, z);  valid: A >= acc_min (false for NaN)
 *   supervised: 1 <= u <= W-2 and 1 <= v <= H-2; the pixel and its four neighbours valid; |z(nb) - z| <= jump_rel z for
 *   each of the four (jump_rel = +inf: the gate is off and nothing is compared); |N| >= normal_min A; |c| > 0
 *   a = X(u+1, v) - X(u-1, v),  b = X(u, v+1) - X(u, v-1),  c = b x a,  rho = 1 - (N / |N|) . (c / |c|)
 *   L = lambda * sum rho / max(S, 1) over the S supervised pixels
 * out3 (device) = {L, sum rho / S, S / (W H)}.  dL_ddepth, dL_dacc [H][W] (each nullable) for upstream gradient 1:
 * dL/dD = g_z / A and dL/dA = -g_z D / A^2, g_z the derivative through the a and b of the pixel's four neighbours; N is
 * data and the gates are steps.  Every element is written, zeros where nothing flows.  Images with W < 3 or H < 3 are
 * legal: no interior, out3 = {0, 0, 0} and zero gradients.
 * Three launches (two without gradients) on the caller's stream, no host synchronisation, no allocation, no atomics,
 * fixed-order reductions: bitwise reproducible.  Profiled under k_lidar_loss_fwd / _finish / _grads (the id word is full).
 * Refused, in this order: height or width < 1; width * height >= 2^31; acc_min, normal_min or lambda negative or NaN;
 * jump_rel negative or NaN; fx or fy not positive and finite; a null depth, acc, normals, out3 or workspace; a float
 * array off 4-byte alignment; the workspace off 8-byte alignment; workspace_bytes below the query (which returns 0 for
 * a refused shape). */
int gsr_blend_attributes(int P, int R, int width, int height, int channels, const float* attributes,
                         const char* geom_buffer, const char* binning_buffer, const char* image_buffer, float* out,
                         void* stream);
int gsr_surfel_normals(int P, const float* xyz, const float* scaling, const float* rotation, const float* T_cw12,
                       float* normals, void* stream);
size_t gsr_normal_consistency_workspace(int height, int width);
int gsr_normal_consistency_loss(int height, int width, const float* depth, const float* acc, const float* normals,
                                float fx, float fy, float cx, float cy, float acc_min, float normal_min,
                                float jump_rel, float lambda, float* out3, float* dL_ddepth, float* dL_dacc,
                                char* workspace, size_t workspace_bytes, void* stream);

/* ---- the delta-depth loss between a history keyframe and its successor (step 5 of optimize_vis), fused ----
 * For every SOURCE pixel (u, v) with d = depth_src[v][u]:
 *   p' = R_rel inv_K_src (u d, v d, d) + t_rel,  Z'[v][u] = p'.z,  (X, Y) = (K_ref p').xy / (K_ref p').z
 *   out[v][u] = bilinear sample of Z' -- the image indexed by SOURCE pixels -- at (X, Y), zero padding, align_corners
 *   a = inv_depth(out), b = inv_depth(depth_ref), inv_depth(x) = x <= 0.01 ? 0 : 1 / x
 *   mask = !(acc_src < 0.5) * !(acc_ref < 0.5),  L = lambda * mean over all H W pixels of |a mask - b mask|
 * replaces GaussianModel::calcDeltaSimi (src/gs/gaussian.cu:116-199), the two inv_depth (include/gs/gs/loss_utils.cuh:
 * 15-21), the masks and the mean of src/liw/lioOptimization.cpp:1780-1801 (lambda_delta_depth_simi of
 * config/basic_common.yaml:65) and their autograd: about forty Torch ops and nine small uploads per pair there, four
 * launches here (three without dL_ddepth_src).  The sampling is the reference's, as it stands (see csrc/delta.hip).
 * depth_*, acc_* (the rendered depth and silhouette of the two views): device [H][W] f32.  inv_K_src9, K_ref9 (3x3) and
 * T_rel12 (3x4, [R_rel | t_rel] = T_ref T_src^-1) are row-major on the HOST and are read before the call returns.
 * out3 (device) = {L, mean gap (L before lambda), share of pixels with mask = 1}.
 * warped (nullable, [H][W]) = out, the image the reference dumps to latest_depth.jpg.
 * dL_ddepth_src / dL_ddepth_ref (nullable, [H][W]) = dL/ddepth for upstream gradient 1, every element WRITTEN; they
 * are the derivative of the forward above (taps and sample coordinates), with sign(0) = 0, no gradient through a
 * clamped inv_depth, and the slope of the cell floor() selects at an integer coordinate.  acc gets no gradient.
 * A sample coordinate that is not finite or beyond +-2^30 is outside the image: value 0, no gradient.
 * Refused (GSR_ERR_INVALID_ARGUMENT, nothing launched or written): height or width < 2, height * width >= 2^31, a null
 * required pointer, workspace_bytes below the query.  The workspace needs no alignment.
 * Deterministic (the many-to-one tap sums are 64-bit integer fixed point, no float atomics, fixed-order reductions),
 * no host synchronisation, no allocation, the caller's stream only. */
size_t gsr_delta_depth_loss_workspace(int height, int width);
int gsr_delta_depth_loss(int height, int width, const float* depth_src, const float* acc_src, const float* depth_ref,
                         const float* acc_ref, const float* inv_K_src9, const float* K_ref9, const float* T_rel12,
                         float lambda, float* out3, float* warped, float* dL_ddepth_src, float* dL_ddepth_ref,
                         char* workspace, size_t workspace_bytes, void* stream);

/* ---- LiDAR depth supervision: a sweep's z-buffer in a keyframe's view, and the masked depth L1 against it ----
 * An extension (the reference compares rendered depths with each other only, and its backward drops dL/ddepth): the
 * consumer of gsr_backward_depth that pins a render to the measured geometry.  Two calls, because they run at
 * different rates: the image once per keyframe, the loss per view per optimiser iteration.
 *
 * gsr_lidar_depth_image: for every point x of points_world (device [n][3] f32)
 *   p = R x + t,  z = p.z,  (X, Y) = (K p).xy / (K p).z,  (ix, iy) = (floor(X + 0.5), floor(Y + 0.5))
 * -- pixel u covers [u - 0.5, u + 0.5), the rasterizer's convention -- and lidar_depth[iy][ix] (device [H][W] f32) is
 * the SMALLEST z of the points of the pixel, 0.0f where there is none; every element is WRITTEN.  T_cw12 (3x4, [R | t],
 * x_c = R x_w + t) and K9 (3x3) are row-major on the HOST and are read before the call returns; K [R | t] is composed
 * in double and rounded once.  A point is dropped when a coordinate of x, z, X or Y is not finite, z <= min_depth,
 * z > max_depth, |X| or |Y| exceeds 2^30 (tested before any conversion to an integer), or the pixel lies outside the
 * image.  counts2 (nullable, device, 2 ints) = {points kept, pixels hit}.  The minimum is a 32-bit integer atomic on
 * the bits of the positive float, taken in the image itself: no workspace, no float atomics, and the image does not
 * depend on the order of the points, bit for bit.  Three launches (one when n == 0, which is legal: an all-zero image
 * and counts2 = {0, 0}).
 * Refused (GSR_ERR_INVALID_ARGUMENT, nothing launched or written): n < 0, height or width < 1, height * width >= 2^31,
 * a null T_cw12, K9 or lidar_depth, a null points_world with n > 0, min_depth not finite or < 0, max_depth not greater
 * than min_depth (+inf is allowed).
 *
 * gsr_lidar_depth_loss: depth = D = sum z alpha T and acc = A = sum alpha T are the rasterizer's second and third
 * outputs (un-normalised), lidar_depth the image above, all device [H][W] f32.  A pixel is SUPERVISED iff
 * lidar_depth > 0 and A >= acc_min (false for NaN); on those pixels e = D / A - lidar_depth and
 *   L = lambda * sum|e| / max(n_sup, 1),   out3 (device) = {L, sum|e| / max(n_sup, 1), n_sup / (H W)}
 * -- the second value is the mean absolute depth error in metres.  dL_ddepth / dL_dacc (nullable, [H][W]) for upstream
 * gradient 1, every element WRITTEN:  dL/dD = c sign(e) / A,  dL/dA = -c sign(e) D / A^2,  c = lambda / n_sup, with
 * sign(0) = 0, exactly 0 on unsupervised pixels, and all zero with out3 = {0, 0, 0} when n_sup == 0.  The normaliser
 * is the supervised count, not H W: the weight of the term does not depend on the density of the sweep.
 * Three launches (two without gradients).
 * Refused (GSR_ERR_INVALID_ARGUMENT, nothing launched or written): height or width < 1, height * width >= 2^31, a null
 * required pointer, acc_min not finite or <= 0, workspace_bytes below the query (the message names the bytes needed).
 * The workspace needs no alignment; the query returns 0 for a refused shape.
 * Both calls: deterministic (fixed-order f64 partial sums narrowed once, integer atomics only), no host
 * synchronisation, no allocation, the caller's stream only. */
int gsr_lidar_depth_image(int n, const float* points_world, const float* T_cw12, const float* K9, int height, int width,
                          float min_depth, float max_depth, float* lidar_depth, int* counts2, void* stream);
size_t gsr_lidar_depth_loss_workspace(int height, int width);
int gsr_lidar_depth_loss(int height, int width, const float* depth, const float* acc, const float* lidar_depth,
                         float acc_min, float lambda, float* out3, float* dL_ddepth, float* dL_dacc, char* workspace,
                         size_t workspace_bytes, void* stream);

/* ---- robust LiDAR depth supervision: the occlusion filter of the supervision image, Huber and clip ----
 * Beside the two calls above, which keep their code and their bits.  The alignment contract is unchanged: float and
 * int32 arrays need 4-byte alignment and nothing more (no 16-byte access is made), the workspace needs none.
 *
 * gsr_lidar_occlusion_filter: lidar_depth and filtered are device [H][W] f32, out of place.  Per pixel, z = lidar_depth[p]:
 *   !(z > 0) (0, negatives, NaN)                       filtered[p] = +0.0f
 *   zmin = the smallest q > 0 of lidar_depth over |dx|, |dy| <= radius around the pixel, the window clamped to the
 *          image and including the pixel itself
 *   zmin < INFINITY && z - zmin > tol * z              filtered[p] = +0.0f (removed: a return seen through a gap of a
 *                                                      nearer surface -- the test of gsr_sweep_admit's code 2, in
 *                                                      float32: one subtraction, one product, one compare)
 *   otherwise                                          filtered[p] = the bits of z
 * Every element is WRITTEN.  counts2 (nullable, device, 2 ints) = {pixels kept, pixels removed}.  radius 0 is a
 * cleaning copy.  One launch (and an 8-byte clear of counts2 on the stream in front of it), no workspace, integer
 * atomics only (the two counts): the output does not depend on the order of anything, bit for bit.
 * Refused (GSR_ERR_INVALID_ARGUMENT, nothing launched or written): height or width < 1, height * width >= 2^31, a null
 * lidar_depth or filtered, radius outside 0..3, tol not finite or < 0, and filtered OVERLAPPING lidar_depth in any
 * byte (the window reads neighbours: the filter cannot run in place).
 *
 * gsr_lidar_depth_loss_robust: gsr_lidar_depth_loss with a quadratic zone near zero and a rejection of outliers.  Per
 * CANDIDATE pixel (lidar_depth > 0 and A >= acc_min, the comparisons of gsr_lidar_depth_loss), with z_L = lidar_depth:
 *   q = D / A,  e = q - z_L,  a = |e|,  tau = huber_abs + huber_rel z_L,  clip = clip_abs + clip_rel z_L
 *   a > clip   CLIPPED: not supervised and not in n_sup, counted in n_clip, both gradients 0 (a NaN a compares false
 *              and stays supervised, as in gsr_lidar_depth_loss)
 *   a < tau    rho = 0.5 a (a / tau),  psi = e / tau
 *   otherwise  rho = a - 0.5 tau,      psi = sign(e), sign(0) = 0
 *   L = lambda * sum rho / max(n_sup, 1)
 *   out4 (device) = {L, sum a / max(n_sup, 1) over the supervised pixels (metres), n_sup / (H W), n_clip / (H W)}
 *   dL/dD = (c psi) / A,  dL/dA = -(dL/dD) q,  c = lambda / n_sup narrowed once; 0 elsewhere; every element WRITTEN.
 * With huber_abs = huber_rel = clip_rel = 0 and clip_abs = +inf, out4[0..2] and both gradients are those of
 * gsr_lidar_depth_loss BIT FOR BIT and out4[3] == 0.  Three launches (two without gradients), deterministic, no host
 * synchronisation, no allocation, no float atomics.
 * Refused as gsr_lidar_depth_loss refuses, and: huber_abs, huber_rel or clip_rel negative, NaN or infinite; clip_abs
 * negative or NaN (+inf is allowed: no clip); workspace_bytes below gsr_lidar_depth_loss_robust_workspace. */
int gsr_lidar_occlusion_filter(int height, int width, const float* lidar_depth, int radius, float tol, float* filtered,
                               int* counts2, void* stream);
size_t gsr_lidar_depth_loss_robust_workspace(int height, int width);
int gsr_lidar_depth_loss_robust(int height, int width, const float* depth, const float* acc, const float* lidar_depth,
                                float acc_min, float lambda, float huber_abs, float huber_rel, float clip_abs,
                                float clip_rel, float* out4, float* dL_ddepth, float* dL_dacc, char* workspace,
                                size_t workspace_bytes, void* stream);

/* ---- sweep admission: the points of a LiDAR sweep that a keyframe's render does not explain yet ----
 * An extension (the reference seeds a voxel once, whatever the map holds, and colours the points on the host from the
 * nearest pixel without an occlusion test): the producer-side step in front of gsr_init_gaussians.
 *
 * gsr_sweep_admit: every point x of points_world (device [n][3] f32) is projected exactly as gsr_lidar_depth_image
 * projects it -- the same T_cw12 / K9 on the HOST, the same composed matrix, the same z, X, Y, ix, iy, bit for bit --
 * and receives ONE reason code, decided in this order:
 *   1 OUT        gsr_lidar_depth_image would drop the point (its rule, min_depth and max_depth included)
 *   2 OCCLUDED   only with lidar_depth (nullable, device [H][W] f32, the image of gsr_lidar_depth_image): zmin = the
 *                smallest POSITIVE value of lidar_depth over |dx|, |dy| <= occlusion_radius around (ix, iy), the window
 *                clamped to the image; the code is 2 iff z - zmin > occlusion_tol * z (never without a positive value)
 *   3 EXPLAINED  only with depth = D = sum z alpha T and acc = A = sum alpha T (nullable TOGETHER, device [H][W] f32,
 *   4 BEHIND     the rasterizer's second and third outputs; absent = no model yet).  If !(A >= acc_min), NaN included,
 *                the silhouette is missing and the point goes on.  Otherwise r = D / A:  r - z > depth_tol * z (the
 *                measurement lies in front of the render): the point goes on;  z - r > depth_tol * z: 4;  anything
 *                else, a NaN r included: 3.  Both comparisons are strict
 *   5 DUPLICATE  only with one_per_pixel != 0: among the points that got this far a pixel keeps the one with the
 *                smallest 64-bit key (bits(z) << 32) | index -- the nearest, and among equal z the lowest index
 *   0 ADMITTED   everything else
 * The admitted points are compacted STABLY (input order).  For the j-th of them, with source index i:
 *   index_out[j] = i;  xyz_out[j] = the three input floats bit for bit;  pixel_out[j] = iy * width + ix and
 *   z_out[j] = z (both nullable)
 *   covs_out[j] = the nine floats of covs_in[i] (nullable, device [n][9]) bit for bit; without covs_in sigma^2 I,
 *     sigma = ((footprint * z) * 2) / (fx + fy), fx = K9[0], fy = K9[4], the off-diagonal elements exact zeros
 *   rgb_out[j] (written only with image: nullable, device [3][H][W] f32 in 0..1): the bilinear sample at (X, Y), pixel
 *     centres at the integers, x0 = floor(X), y0 = floor(Y), the four taps clamped to the image (border replication),
 *     two horizontal lerps then one vertical, each a + t * (b - a); with exposure (nullable, device [3][2], rows
 *     (g, b) as gsr_apply_exposure takes them) inverted, (v - b) / g; then times 255.  No clamp
 * Rows j >= admitted of every output are NOT written (each output holds n rows).  reasons (nullable, device n bytes)
 * is written in every element; counts6 (device, 6 ints) = {admitted, out, occluded, explained, behind, duplicate},
 * which sum to n.  n == 0 is legal: counts6 all zero, nothing else written, no workspace needed.
 * Five launches (four without one_per_pixel, one when n == 0), 64-bit and 32-bit INTEGER atomics only (the minimum
 * commutes: the same bits on every run), no host synchronisation, no allocation, the caller's stream only.
 * Refused (GSR_ERR_INVALID_ARGUMENT, nothing launched or written), in this order: n < 0; height or width < 1;
 * height * width >= 2^31; a null T_cw12, K9, xyz_out, covs_out, index_out or counts6, or a null points_world with
 * n > 0; depth without acc or acc without depth; acc_min not finite or <= 0; depth_tol, occlusion_tol or footprint not
 * finite or < 0; occlusion_radius outside 0..3; min_depth not finite or < 0; max_depth not greater than min_depth (+inf
 * is allowed); workspace_bytes below the query (the message names the bytes needed); a null workspace with n > 0; a
 * float or int32 array off 4-byte alignment.  The workspace needs no alignment; the query returns 0 for a refused
 * shape (and for n == 0). */
size_t gsr_sweep_admit_workspace(int n, int height, int width);
int gsr_sweep_admit(int n, const float* points_world, const float* covs_in, const float* T_cw12, const float* K9,
                    int height, int width, float min_depth, float max_depth, const float* depth, const float* acc,
                    float acc_min, float depth_tol, const float* lidar_depth, int occlusion_radius,
                    float occlusion_tol, const float* image, const float* exposure, float footprint,
                    int one_per_pixel, float* xyz_out, float* covs_out, float* rgb_out, int* index_out, int* pixel_out,
                    float* z_out, unsigned char* reasons, int* counts6, char* workspace, size_t workspace_bytes,
                    void* stream);

/* ---- the sweep voxel map: fused voxel moments and one oriented Gaussian per matured voxel ----
 * An extension between gsr_sweep_admit and gsr_init_gaussians: where the reference voxelises a sweep with a serial
 * unordered_map walk on the host (GpMap::splitPointsIntoCell / dividePointsIntoCellInitMap, src/gp3d/map.cpp) and runs
 * a Gaussian-process regression per voxel, this keeps a PERSISTENT voxel table on the device with exact,
 * order-independent moments and seeds ONE oriented Gaussian (a surfel) per voxel from them.
 *
 * Definitions, with g = (double)grid and Q = 2^20, for a point p (three f32):
 *   t_k = (double)p_k / g,  c_k = floor(t_k)  (floor, not truncation: -1e-9 lies in cell -1);  the point is OUT when a
 *     t_k is not finite or |c_k| >= Q
 *   key = ((c_x + Q) << 42) | ((c_y + Q) << 21) | (c_z + Q): injective, positive, never 0 (0 marks an empty slot)
 *   q_k = min(Q - 1, (int64)floor((t_k - c_k) * Q))  (the clamp matters: for p = -1e-30, t - c rounds to 1.0)
 *   per voxel, unsigned 64-bit, added with INTEGER atomics only: count;  S1[3] = sum q_k;  S2[6] = sum q_i q_j in the
 *     order (xx, xy, xz, yy, yz, zz);  with colors (nullable, device [n][3] f32, 0..255):
 *     SC[3] = sum clamp(llrint(c * 256), 0, 65535), a NaN counting as 0
 *   Integer addition commutes: the sums are the same bits for every thread order and every permutation of the sweep.
 *   n <= 2^22 per call, min_points <= 2^20 and a matured voxel closes, so count < 2^23 and S2 < 2^63.
 *   From the sums, in float64, uncontracted, in this order:
 *     a_k = S1_k / count;  mean m_k = (c_k + (a_k + 0.5) / Q) * g
 *     population covariance C_ij = (S2_ij / count - a_i * a_j) * ((g / Q) * (g / Q));  colour SC / (256 * count)
 *
 * The table is the caller's: capacity slots of 16 int64 (128 bytes: key, closed, count, S1, S2, SC, and a word that is
 * zero between calls), capacity a power of two up to 2^26, ZEROED before its first use, 8-byte aligned.
 * gsr_voxel_table_bytes(capacity) = 128 * capacity, or 0 for a refused capacity.
 *
 * gsr_voxel_sweep: one call per sweep, four launches (one when n == 0), no host synchronisation, no allocation.
 *   insert   every point finds or claims its voxel's slot (open addressing, 64-bit compare-and-swap on the key, at
 *            most `capacity` probes) and gets status[i] (device, n bytes) and point_keys[i] (device int64, -1 for OUT):
 *              0 ACCUMULATED  the sums above were added
 *              1 SEEDED       the voxel matured in an EARLIER call: nothing changes (a similarity-loss point)
 *              2 OUT          out of range or not finite
 *              3 FULL         no slot within `capacity` probes: nothing changes
 *            The status is decided by the closed flag as the previous call left it; nothing in the call's insert
 *            writes that flag.  Below a full table both outputs are deterministic; slot numbers are never exposed.
 *   harvest  a voxel matures when this call accumulated into it and count >= min_points.  The matured voxels are
 *            emitted in the order of their smallest point index in this call -- the order of first appearance -- and
 *            closed.  Row j of the outputs (each holds n rows; rows at and behind the matured count are NOT written):
 *              xyz_out[j]       the mean;  keys_out[j] the key (int64);  points_out[j] the count
 *              covs_out[j]      [3][3] f32, symmetric: V diag(lam) V^T, lam the eigenvalues of C in DESCENDING order,
 *                               each clamped below at min_sigma^2, V's columns the axes, made right-handed (cyclic
 *                               Jacobi in float64, a fixed number of sweeps: the same bits on every run)
 *              scaling_out[j]   log(sqrt(lam * scale_factor)): gsr_init_gaussians' scaling of a diagonal covariance
 *              rotation_out[j]  the quaternion (w, x, y, z), w >= 0, normalised, of the rotation R whose columns are
 *                               the axes: Sigma = R S^2 R^T, what the rasterizer builds from (scale, rotation)
 *              normal_out[j]    the axis of the smallest eigenvalue (its sign is arbitrary)
 *              rgb_out[j]       the colour, written only with colors
 *   counts6 (device, 6 ints) = {accumulated, seeded, out, full, matured, live keys}; the first four sum to n; live keys
 *   = live_before + the keys this call inserted, live_before being what the previous call on this table reported
 *   (0 for a zeroed table, unchanged by gsr_voxel_rehash).
 * Keep live keys + n <= capacity / 2 (grow with gsr_voxel_rehash first) and no point is ever FULL.
 * gsr_voxel_sweep_workspace(n): the bytes of workspace the call needs (0 for n == 0 or a refused n); any alignment.
 *
 * gsr_voxel_rehash: every record of src into dst, a ZEROED table that is not smaller; one launch, one thread per source
 * slot.  The two tables hold the same records afterwards.
 *
 * Refused (GSR_ERR_INVALID_ARGUMENT, nothing launched or written), in this order: n outside 0..2^22; min_points
 * outside 1..2^20; grid, min_sigma or scale_factor not finite or <= 0; capacity not a power of two in 1..2^26;
 * live_before outside 0..capacity; a null table or counts6, or with n > 0 a null points, status, point_keys or seed
 * output (rgb_out only with colors); workspace_bytes below the query; a null workspace with n > 0; a float or int32
 * array off 4-byte alignment; the table, point_keys or keys_out off 8-byte alignment.  gsr_voxel_rehash: a refused
 * capacity; capacity_dst < capacity_src; a null or misaligned table; src == dst. */
size_t gsr_voxel_table_bytes(long long capacity);
size_t gsr_voxel_sweep_workspace(int n);
int gsr_voxel_sweep(int n, const float* points, const float* colors, float grid, int min_points, float min_sigma,
                    float scale_factor, long long* table, long long capacity, int live_before, unsigned char* status,
                    long long* point_keys, float* xyz_out, float* covs_out, float* rgb_out, long long* keys_out,
                    int* points_out, float* scaling_out, float* rotation_out, float* normal_out, int* counts6,
                    char* workspace, size_t workspace_bytes, void* stream);
int gsr_voxel_rehash(const long long* src, long long capacity_src, long long* dst, long long capacity_dst,
                     void* stream);

/* ---- the evaluation pass around a forward-only render: PSNR, SSIM and 8-bit frame export ----
 * gsr_image_metrics: out4 (device) = {psnr, ssim, l1, mse} of img against gt, [channels][H][W] device f32, in two
 * launches:
 *   mse_c = mean over H W of (img - gt)^2 in channel c,  psnr = mean_c 20 log10(1 / sqrt(mse_c)),  mse = mean_c mse_c
 *   ssim = mean(SSIM(img, gt)), l1 = mean|img - gt|: the arithmetic of gsr_photometric_loss, same window convention
 * replaces gaussian_splatting::psnr and ::ssim (include/gs/gs/loss_utils.cuh:89-93, 43-70) as saveRender calls them per
 * keyframe (src/liw/lioOptimization.cpp:2203-2207) and the status line of optimize_vis every 50 iterations
 * (:1739-1776).  psnr is the reference's, as it stands: the MEAN OF THE PER-CHANNEL PSNRs, not the PSNR of the pooled
 * error; it is evaluated in float64 from fixed-order float64 sums and narrowed once; a channel with mse_c == 0 makes it
 * +inf, as 1.0 / 0 does there.  Nothing is stored per pixel: the workspace holds three floats per 54 x 32 work unit and
 * needs no more than float alignment.
 * totals (nullable, device, 4 doubles, 8-byte aligned): {(double)out4[0], (double)out4[1], (double)out4[2], 1.0} is
 * ADDED to it -- the values as stored, widened -- so that after a keyframe sweep into one zeroed buffer it holds
 * exactly the float64 sums of the per-frame psnr, ssim and l1 in stream order and the frame count (saveRender's
 * psnr_value / ssim_value / count, :2184-2231, without its two .item() round trips per frame).  An infinite frame
 * makes that sum infinite, as there.
 * Refused (GSR_ERR_INVALID_ARGUMENT, nothing launched or written), in this order: a non-positive dimension; H * W >=
 * 2^31 - 1; a null img, gt, window11_host, out4 or workspace; workspace_bytes below the query (the message names the
 * bytes needed).  The query returns 0 for a refused shape.  Deterministic, no host synchronisation, no allocation,
 * the caller's stream only.
 *
 * gsr_pack_image_u8: img3 [3][H][W] device f32 -> out, interleaved 8-bit [H][W][3] whose rows are pitch_bytes apart:
 * v = x * 255 in float32, clamped to [0, 255], truncated toward zero; NaN -> 0 (the reference leaves that cast
 * undefined).  bgr = 0: out[..][c] = plane c; bgr = 1: planes 2, 1, 0 -- what tensor2CvMat3X (:2113-2136:
 * mul(255).clamp(0, 255).to(kU8) and the channel swap for cv::imwrite) returns.  The bytes between a row's 3 W bytes and
 * the next row are never written, so the hconcat of :2219-2220 is two calls into one [H][2 W][3] buffer (out + 3 W for
 * the right half, pitch 6 W).  Any out address and any pitch >= 3 W are accepted (4-byte stores are used where they
 * allow it).  Refused: a non-positive dimension; H * W >= 2^31 - 1; a null pointer; pitch_bytes < 3 W.
 *
 * gsr_pack_depth_u8: depth [H][W] device f32 -> out, 8-bit [H][W] with a row pitch: round-half-to-even of
 * depth * (255 / max_depth), the factor formed and the multiply done in float32, saturated to [0, 255], NaN -> 0 --
 * cv::Mat::convertTo(CV_8U) as OpenCV documents it, i.e. tensor2CvMat2X (:2150-2164) up to its colour map, which
 * stays on the host.  Refused: as above with pitch_bytes < W, and max_depth not positive and finite. */
size_t gsr_image_metrics_workspace(int channels, int height, int width);
int gsr_image_metrics(int channels, int height, int width, const float* img, const float* gt,
                      const float* window11_host, float* out4, double* totals, char* workspace, size_t workspace_bytes,
                      void* stream);
int gsr_pack_image_u8(int height, int width, const float* img3, int bgr, unsigned char* out, size_t pitch_bytes,
                      void* stream);
int gsr_pack_depth_u8(int height, int width, const float* depth, float max_depth, unsigned char* out,
                      size_t pitch_bytes, void* stream);

/* ---- "next" row: the data formats either side of the path ----
 * gsr_init_gaussians: new map points -> leaf parameter rows, the arithmetic of GaussianModel::addNewPointcloud
 * (src/gs/gaussian.cu:241-313): _xyz = xyz; _scaling = log(sqrt(diag(cov) * scale_factor)) (decomposeSR keeps the
 * diagonal, :10-11, 276-281); _rotation = (1, 0, 0, 0); _opacity = inverse_sigmoid(0.5) = 0;
 * _features_dc[.][0][c] = (rgb_c / 255 - 0.5) / C0; _features_rest = 0.  covs [n][3][3], rgbs [n][3] in 0..255.
 * The *_out pointers address row `P_old` of the caller's capacity buffers: rows are initialised in place, so
 * growing the map moves O(n) bytes instead of re-concatenating all six tensors and their Adam moments
 * (densification_postfix / cat_tensors_to_optimizer, :451-472, 524-540).
 * gsr_pack_ply_rows: the vertex rows of the reference's PLY export (construct_list_of_attributes :474-492,
 * Save_ply :494-522): per Gaussian gsr_ply_row_floats(M) = 14 + 3M little-endian f32 --
 *   x y z | nx ny nz (zeros) | f_dc_0..2 | f_rest_0..3(M-1)-1 | opacity | scale_0..2 | rot_0..3
 * with f_dc / f_rest in the reference's transpose(1,2).flatten(1) (channel-major) order.  rows: device buffer of
 * P * (14 + 3M) floats; the host copies it once and writes header + rows (gs-livm_amd/ply.py). */
int gsr_init_gaussians(int n, int M, const float* xyz, const float* covs, const float* rgbs, float scale_factor,
                       float* xyz_out, float* features_dc_out, float* features_rest_out, float* scaling_out,
                       float* rotation_out, float* opacity_out, void* stream);
size_t gsr_ply_row_floats(int M);
int gsr_pack_ply_rows(int P, int M, const float* xyz, const float* features_dc, const float* features_rest,
                      const float* opacity, const float* scaling, const float* rotation, float* rows, void* stream);

/* ---- in-place pruning: the rows that no optimiser step brings back leave the model (an extension) ----
 * The other half of the optimiser-state surgery: GaussianModel::prune_optimizer (src/gs/gaussian.cu:430-449) is an
 * index_select of a leaf and of both of its Adam moments, per group; the reference carries it and never calls it.
 * Removal is a STABLE compaction: surviving rows keep their relative order (a voxel's row range stays a range; the
 * rasterizer breaks depth ties by ascending row number).
 *
 * gsr_prune_mark (three launches): reasons[P] (uint8, 0 = keep) and the row map of the compaction.  Drop bits:
 *   bit 0  sigmoid(opacity_raw) < min_opacity      (below 1/255 a row's alpha never reaches the blend's 1/255 test)
 *   bit 1  any exp(scaling_raw[k]) > max_scale     (k_preprocess' scale cull at scale_modifier 1, forward.cu:19-25)
 *   bit 2  drop_nonfinite != 0 and any of xyz, scaling_raw, rotation_raw, opacity_raw is NaN or +-Inf (a NaN compares
 *          false in both tests above and would otherwise stay for ever).  Such a row is NOT invisible to gsr_forward
 *          ("Non-finite inputs" above): dropping it changes the pixels it painted.
 *   bit 3  drop (nullable, [P] bytes) is non-zero: the caller's own mask
 * The activated values are gsr_activate's bit for bit; a value ON a threshold is kept (the rasterizer culls on >).
 *   row_map [P + 1] int32: the exclusive prefix sum of "kept" -- row_map[i] is the new row of old row i (for a dropped
 *     row: the new row of the next survivor), row_map[P] = P', the new row count;
 *   counts5 [5] int32 = {P', rows with bit 0, with bit 1, with bit 2, with bit 3} (a row counts under each of its bits).
 * xyz [P][3], scaling_raw [P][3], rotation_raw [P][4], opacity_raw [P]: the raw leaves.  workspace: gsr_prune_workspace(P)
 * bytes -- five int32 per 256 rows, nothing per row.
 * gsr_prune_compact (ONE launch for all tensors, whatever P): for up to 18 tensors -- six leaves x {parameter, exp_avg,
 * exp_avg_sq} -- of widths[k] floats per row, dst[k][row_map[i]] = src[k][i] for every row with reasons[i] == 0.  src
 * and dst are HOST arrays of device pointers; a destination is a buffer of its own of at least row_map[P] rows (out of
 * place: an in-place stable compaction races), rows [row_map[P], ...) of it are not written.  A tensor of width 0
 * (_features_rest at M = 1) is skipped and its pointers are not looked at.
 * Alignment of caller tensors: they are contiguous and need only the alignment of their element, 4 bytes (reasons and
 * drop: 1) -- every access is an element access.  A pointer at any other offset is refused.
 * Refused (GSR_ERR_INVALID_ARGUMENT, nothing enqueued or written), in this order: shape (P < 0 or P > GSR_PRUNE_MAX_ROWS;
 * compact: more than 18 tensors, a negative width, a model beyond one launch's 2^31 - 1 workgroups of 1024 floats); a
 * null required pointer; a misaligned pointer; workspace_bytes below the query (the message names the bytes needed).
 * P == 0: no row is touched; gsr_prune_mark writes row_map[0] = 0 and counts5 = {0, ...} (only those two are required),
 * gsr_prune_compact returns at once.  The query returns 0 for P <= 0 and for a refused P.
 * Deterministic (no atomics, no workgroup waits for another), no host synchronisation, no allocation, the caller's
 * stream only. */
#define GSR_PRUNE_MAX_ROWS 0x7fffff00
size_t gsr_prune_workspace(int P);
int gsr_prune_mark(int P, const float* xyz, const float* scaling_raw, const float* rotation_raw,
                   const float* opacity_raw, const unsigned char* drop, float min_opacity, float max_scale,
                   int drop_nonfinite, unsigned char* reasons, int* row_map, int* counts5, char* workspace,
                   size_t workspace_bytes, void* stream);
int gsr_prune_compact(int P, int n_tensors, const float* const* src, float* const* dst, const int* widths,
                      const unsigned char* reasons, const int* row_map, void* stream);

/* ---- adaptive density control: clone and split where the photometric gradient asks for it (an extension) ----
 * The growing counterpart of pruning.  The reference carries the remains of it (densification_postfix,
 * src/gs/gaussian.cu:521-540; the commented _xyz_gradient_accum / _max_radii2D, :362, :398, :535-537;
 * cat_tensors_to_optimizer, :451-472) and never runs the loop; the rule is upstream 3D Gaussian splatting's
 * densify_and_clone / densify_and_split with N = 2.  When to densify and with which thresholds stays with the caller.
 *
 * stats [P][3] f32, one row per Gaussian: {grad_sum, views, max_radius} -- all floats, so that gsr_prune_compact moves
 * the row as one tensor of width 3 (counts and radii stay far below 2^24).
 *
 * gsr_density_accumulate (ONE launch per view, after that view's gsr_backward): for a row with radii[i] > 0 and a
 * finite n = sqrtf(gx * gx + gy * gy): grad_sum += n, views += 1, max_radius = max(max_radius, (float)radii[i]); any
 * other row is not touched.  gx, gy are dL_dmean2D[i][0], [i][1] exactly as gsr_backward writes them -- the quantity
 * upstream's viewspace_point_tensor.grad carries; NO rescaling (by the image size or otherwise) is applied, and
 * grad_threshold below is in those units.  radii [P] int32 is the forward's output.  The products, the sum, the square
 * root and the additions are single float32 operations (no contraction), so a host restates the row bit for bit.
 *
 * gsr_densify_mark (three launches).  Per row: avg = views > 0 ? grad_sum / views : 0.  The row is a CANDIDATE iff
 * avg >= grad_threshold (upstream's >=; a NaN compares false) and all three scaling_raw entries are finite.  A
 * candidate is BIG iff max_k expf(scaling_raw[k]) > size_threshold -- gsr_activate's expf bit for bit, the comparison
 * strict as in the prune rule (a scale ON the threshold is not big).
 *   kinds [P] uint8: 0 = none, 1 = clone (candidate, not big), 2 = split (candidate, big).
 *   Every candidate adds exactly ONE row.  offsets [P + 1] int32: the exclusive prefix sum of "candidate", capped at
 *   max_new (max_new < 0: unlimited); offsets[P] = n_new.  A candidate whose uncapped offset is >= max_new gets kind 0:
 *   THE FIRST max_new CANDIDATES IN ROW ORDER WIN.
 *   counts3 [3] int32 = {n_new, clones accepted, splits accepted}.
 * workspace: gsr_densify_workspace(P) bytes -- two int32 per 256 rows, nothing per row beyond the two outputs.
 *
 * gsr_densify_apply (ONE launch, one thread per source row), in place on capacity buffers that the caller guarantees
 * to hold P + n_new rows; kinds / offsets / n_new = offsets[P] are gsr_densify_mark's.  The six leaves are the raw
 * parameters xyz [.][3], features_dc [.][1][3], features_rest [.][M-1][3], scaling_raw [.][3], rotation_raw [.][4],
 * opacity_raw [.][1]; exp_avg6 / exp_avg_sq6 are HOST arrays of six device pointers in that order (each array may be
 * null as a whole: no moments of that kind), stats may be null.  At M = 1 features_rest and entry [2] of the moment
 * arrays are not looked at.  With j = P + offsets[i]:
 *   kind 1, clone: row j of all six leaves = row i, bit for bit; both moments of row j are WRITTEN as zeros in all six
 *     groups; stats row j = 0; row i, its moments and its stats row are untouched (upstream's clone: the parent keeps its
 *     optimiser state, the copy starts fresh).
 *   kind 2, split (upstream's N = 2, laid out without a compaction): the parent row i becomes child 0 IN PLACE -- every
 *     existing row keeps its number and child 0 stays inside its voxel's row range -- and child 1 is written to row j.
 *     xyz_c = xyz_i + R (sigma * z_c), sigma_k = expf(scaling_raw[i][k]), R the rotation matrix of the quaternion as
 *     gsr_activate normalises it (q / max(|q|, 1e-12), component order w, x, y, z); scaling_c = scaling_raw[i] -
 *     0.47000363f (ln 1.6 = upstream's log(scale / (0.8 N)) with one rounding); rotation, opacity and all SH rows are
 *     copied; both moments of rows i AND j are zero in all six groups (upstream's children are fresh parameters); the
 *     stats rows i and j are zero.
 *   kind 0: the row is not read beyond kinds[i].  No row >= P + n_new is written.
 * The normals z_c come from a counter-based generator, so that any host can restate them: Philox4x32-10 (multipliers
 * D2511F53, CD9E8D57; key increments 9E3779B9, BB67AE85) with key = (seed & 0xffffffff, seed >> 32) and counter =
 * (i, c, 0, 0) gives o_0..o_3; u_k = ((o_k >> 9) + 0.5) * 2^-23 -- exact in float32 (2n + 1 < 2^24) and strictly inside
 * (0, 1), u >= 2^-24; r1 = sqrtf(-2 logf(u_0)), t1 = 6.2831855f * u_1, r2 = sqrtf(-2 logf(u_2)), t2 = 6.2831855f * u_3;
 * z = (r1 cosf(t1), r1 sinf(t1), r2 cosf(t2)).  (23 bits rather than 24: with 24, n + 0.5 needs 25 significant bits
 * for n >= 2^23 and would be rounded.)  A child depends on (seed, i, c) and its own row only: bitwise reproducible,
 * independent of P, of the launch shape and of which other rows are marked.
 * Alignment: contiguous tensors at their element's alignment, 4 bytes (kinds: 1); any other offset is refused.
 * Refused (GSR_ERR_INVALID_ARGUMENT, nothing enqueued or written), in this order: shape (P < 0, P or P + n_new beyond
 * GSR_PRUNE_MAX_ROWS, n_new < 0, M outside 1..16); a null required pointer; a misaligned pointer; workspace_bytes
 * below the query (the message names the bytes needed).  P == 0 and n_new == 0 are legal and touch no row:
 * gsr_densify_mark then writes offsets[0] = 0 and counts3 = {0, 0, 0} (only those two are required), the other two
 * return at once.  The query returns 0 for P <= 0 and for a refused P.
 * Deterministic (no atomics, no workgroup waits for another), no host synchronisation, no allocation, the caller's
 * stream only. */
int gsr_density_accumulate(int P, const int* radii, const float* dL_dmean2D, float* stats, void* stream);
size_t gsr_densify_workspace(int P);
int gsr_densify_mark(int P, const float* stats, const float* scaling_raw, float grad_threshold, float size_threshold,
                     int max_new, unsigned char* kinds, int* offsets, int* counts3, char* workspace,
                     size_t workspace_bytes, void* stream);
int gsr_densify_apply(int P, int M, int n_new, const unsigned char* kinds, const int* offsets, unsigned long long seed,
                      float* xyz, float* features_dc, float* features_rest, float* scaling_raw, float* rotation_raw,
                      float* opacity_raw, float* const* exp_avg6, float* const* exp_avg_sq6, float* stats,
                      void* stream);

/* ---- keyframe covisibility: one bit per (keyframe, Gaussian), kept on the device (an extension) ----
 * The reference draws its training views blindly (lioOptimization.cpp:1573-1641).  A host that refines poses and prunes
 * floaters wants what MonoGS and SplaTAM keep: which keyframes see the same Gaussians, and how many keyframes see each
 * Gaussian.  Which keyframes to choose, with which thresholds, and when to prune stays with the caller.
 *
 * A VISIBILITY ROW is `words` >= gsr_visibility_words(P) little-endian 64-bit words: bit i % 64 of word i / 64 belongs
 * to model row i.  The rows of several keyframes lie in one SLAB with a row pitch counted in words (pitch >= words; the
 * words between a row's end and the next row are never read or written).  Everything here is integer arithmetic: every
 * result is exact and the same on every run.
 *
 * gsr_visibility_pack (ONE launch per keyframe): bit i = radii[i] > 0 (radii [P] int32, gsr_forward's output) or
 * mask[i] != 0 (mask [P] bytes, what gsr_mark_visible writes); exactly one of the two is given.  ALL `words` words of the
 * row are written and the bits at and beyond P are zero: a row recorded again after the model shrank or grew carries no
 * stale bit.
 *
 * gsr_covisibility (ONE launch behind the zero fill of the outputs on the stream): for Q query rows and K keyframe rows
 * over `words` words, inter [Q][K] int32 (row-major) = sum over the words of popcount(q_w & k_w); q_count [Q] and
 * k_count [K] (each nullable) are the rows' own popcounts.  The two slabs may be the same memory: the full matrix, whose
 * diagonal is the counts.  Eight query rows stay in registers while the keyframe rows stream past them, so a keyframe
 * word is loaded once per eight query rows.  Per-workgroup partial counts are added with 32-bit integer atomics: exact
 * and independent of the order.  All `words` words count: a caller that passes more than gsr_visibility_words(P) words
 * keeps the tail zero, as gsr_visibility_pack does.
 *
 * gsr_observation_count (ONE launch, each word of the slab read once): count [P] int32 (nullable) = how many of the K
 * rows have bit i set; drop [P] bytes (nullable) = (i >= first_row && count[i] < min_count) ? 1 : 0 -- the mask
 * gsr_prune_mark takes as `drop`: the rows from first_row on that fewer than min_count keyframes observe.  At least one
 * of the two is asked for.
 *
 * gsr_visibility_remap (ONE launch) follows a stable compaction: reasons [P] and row_map [P + 1] exactly as
 * gsr_prune_mark wrote them, on the device.  In each of the K destination rows bit row_map[i] = source bit i for every
 * row with reasons[i] == 0, and every other bit of the row's dst_words words is zero.  Out of place; a gather (each
 * destination word is stored once: no atomics, no separate zero fill).  The new row count P' = row_map[P] is known to
 * the device only: the caller passes dst_words >= gsr_visibility_words(P') -- gsr_visibility_words(P) always suffices
 * -- and a bit that would lie beyond dst_words words is not written anywhere.
 *
 * Alignment: visibility words 8 bytes, int32 arrays 4 bytes, byte arrays 1; any other offset is refused.
 * Refused (GSR_ERR_INVALID_ARGUMENT with a gsr_last_error text, nothing enqueued or written), IN THIS ORDER:
 *   1. shape: a count (P, Q, K, words, dst_words) that is not positive; `words` or a pitch below what the rows need
 *      (gsr_visibility_words(P); `words`; dst_words); words * 64 beyond int32; Q * K beyond int32; a negative first_row or
 *      min_count;
 *   2. the choice: both or neither of radii and mask; neither of count and drop;
 *   3. a null required pointer (q_count and k_count are optional);
 *   4. a misaligned pointer, bit pointers before int32 pointers;
 *   5. gsr_visibility_remap: src and dst slabs that overlap.
 * gsr_visibility_words(P) = (P + 63) / 64, 0 for P <= 0.
 * No host synchronisation, no allocation, the caller's stream only. */
size_t gsr_visibility_words(int P);
int gsr_visibility_pack(int P, const int* radii, const unsigned char* mask, unsigned long long* bits, int words,
                        void* stream);
int gsr_covisibility(int Q, const unsigned long long* q_bits, long long q_pitch, int K,
                     const unsigned long long* k_bits, long long k_pitch, int words, int* inter, int* q_count,
                     int* k_count, void* stream);
int gsr_observation_count(int K, const unsigned long long* bits, long long pitch, int P, int first_row, int min_count,
                          int* count, unsigned char* drop, void* stream);
int gsr_visibility_remap(int K, const unsigned long long* src, long long src_pitch, int P,
                         const unsigned char* reasons, const int* row_map, unsigned long long* dst, long long dst_pitch,
                         int dst_words, void* stream);

/* ---- per-Gaussian blend contribution: pixels, weight sum, largest weight (an extension) ----
 * radii > 0 says that a Gaussian is in the frustum, not scale-culled and non-degenerate; it does not say that the
 * Gaussian put anything into a pixel (a splat behind a wall of opaque ones has radii > 0 and contributes nothing).
 * MonoGS builds covisibility and pruning on n_touched, the number of pixels a Gaussian contributed to; the reference's
 * rasterizer has no such output.  This is a forward-only pass behind gsr_forward over the three blobs that forward left
 * (it reads the tile ranges of both segments, point_list, the splat records, n_contrib and quad_last: no model tensor,
 * no image, no background), so it works for one-chain and near/far frames and in both binning modes: the blobs carry
 * the mode.  It is off unless called.
 *
 * A pixel TAKES the splat at position pos of its tile's list iff pos < n_contrib[pixel] (the forward's own termination
 * cut), power <= 0 and alpha = min(0.99, opacity exp(power)) >= 1/255, with alpha recomputed by the blend's own device
 * functions: exactly the (pixel, splat) pairs the forward blended.  Pixels outside the image never count.  Per
 * Gaussian, over the pixels that take it:
 *   n_touched   the number of those pixels;
 *   weight_sum  sum of alpha T, T = the transmittance in front of the splat, carried front to back from 1 as the
 *               forward carries it (the Gaussian's share of out_acc: the sums of all rows add up to sum out_acc);
 *   weight_max  max of alpha T.
 *
 * gsr_contribution (the zero fill of frame_rows on the stream plus ONE launch; P, R, width, height as gsr_backward takes
 * them, R = what gsr_forward returned) writes frame_rows, P rows of 16 bytes {u64 wsum_fx, u32 pixels, u32 wmax_bits}:
 * a tile's weight sum is added over the tile's pixels in a fixed order in float32, rounded to units of 2^-32 and added
 * to wsum_fx with a 64-bit integer atomic; the count with a 32-bit integer atomic; the maximum with an integer atomic
 * max on the bits of the non-negative float.  The rows are therefore bitwise reproducible and independent of the order
 * the tiles run in.  One frame cannot overflow them (pixels <= width * height < 2^31, wsum_fx < width * height * 2^32).
 * P == 0 and R == 0 are legal: nothing is launched and (R == 0) the rows are zero; with R == 0 the blobs are not read
 * and may be NULL.  gsr_contribution_workspace(P) = 16 * P bytes, 0 for P <= 0.
 *
 * gsr_contribution_finish (ONE launch, one thread per row) turns the rows into the outputs, each nullable:
 *   n_touched [P] int32; weight_sum [P] f32 = (float)((double)wsum_fx * 2^-32); weight_max [P] f32;
 *   mask [P] bytes = (n_touched >= min_pixels && weight_max >= min_weight) ? 1 : 0 -- what gsr_visibility_pack takes
 *   as `mask`;
 *   stats [P][3] f32 = {weight_sum_total, views, weight_max}, UPDATED in place: [0] += weight_sum, [1] += 1 where
 *   n_touched > 0, [2] = max([2], weight_max) -- all floats, so that gsr_prune_compact moves the rows as one tensor of
 *   width 3, the convention of the density statistics.
 * Every element of every requested output is written, rows with radii <= 0 included: no tile lists them, they read 0.
 *
 * Refused (GSR_ERR_INVALID_ARGUMENT with a gsr_last_error text, nothing enqueued or written), IN THIS ORDER:
 *   1. shape: a negative P or R, width or height not positive, width * height >= 2^31; a negative min_pixels, a
 *      min_weight that is negative or NaN;
 *   2. gsr_contribution_finish: none of the five outputs is asked for;
 *   3. a null required pointer (P > 0: frame_rows; R > 0 as well: the three blobs);
 *   4. a misaligned pointer: frame_rows 8 bytes, then the int32 / float arrays 4 bytes (mask: any address).
 * No host synchronisation, no allocation, the caller's stream only.  Timed under the profiler id "k_visibility". */
size_t gsr_contribution_workspace(int P);
int gsr_contribution(int P, int R, int width, int height, const char* geom_buffer, const char* binning_buffer,
                     const char* image_buffer, char* frame_rows, void* stream);
int gsr_contribution_finish(int P, const char* frame_rows, int min_pixels, float min_weight, int* n_touched,
                            float* weight_sum, float* weight_max, unsigned char* mask, float* stats, void* stream);

/* Optional per-kernel device timing (hipEvent pairs recorded on the launch stream around every
 * kernel launch while enabled).  Measurement aid for bench.py's roofline line; the reference has only
 * host wall-clock timers (include/common/timer/timer.h:36-52).  Not thread-safe; off by default.
 *   (the event pool is guarded by a mutex; enabling / reading while other threads launch is safe, the
 *   attribution of events to forwards of concurrent threads is then simply interleaved)
 *   gsr_profile_enable(1) starts a fresh recording, gsr_profile_enable(0) stops it.
 *   gsr_profile_read synchronises the recorded events, writes per-kernel total milliseconds and launch
 *   counts for kernel ids [0, gsr_kernel_count()), clears the recording, returns the number of ids written. */
int gsr_kernel_count(void);
const char* gsr_kernel_name(int kernel_id);
int gsr_profile_enable(int on);
/* like gsr_profile_enable(1), but records only the listed kernel ids: an event pair costs a few microseconds
 * of GPU idle time per launch, so a timed run should carry events for the kernel under study only.
 * The set of recorded ids is one 64-bit word and gsr_kernel_count() is 64: THE WORD IS FULL.  The four covisibility
 * kernels are timed under the one id "k_visibility"; the next kernel shares an id or widens the word first. */
int gsr_profile_enable_only(const int* kernel_ids, int n);
int gsr_profile_read(int max_ids, double* total_ms, int* launches);
/* diagnostics: number of gsr_forward calls of this process whose instance count reached the host through the
 * fallback stream query instead of the polled mailbox word (0 in a healthy run; each one leaves the GPU idle for up
 * to one query period, 25 us). */
unsigned long long gsr_mailbox_slow_path_hits(void);
/* ... and what the most recent such exit saw: the ticket it waited for, the ticket in the word at the last spin
 * and right after the first successful hipStreamQuery, the time since the enqueue, and whether the word was
 * already there when that HIP call returned (1 = the count was only invisible to the spinning load until a HIP
 * call was made; 0 = the store itself arrived after the stream had drained).  count = 0: never happened. */
typedef struct gsr_mailbox_event {
  unsigned count;
  uint32_t ticket_expected, ticket_seen_before_query;
  double elapsed_us;
  uint32_t ticket_seen_after_query;
  int first_query_result;
  int visible_at_query;
  /* how the wait was spent: stream queries made before the one that found the stream drained, the longest any single
   * query took to RETURN, and the longest the host went without getting to run (gap between two polls of the word):
   * a drained-late stream shows many quick queries, a stalled driver call one long query, a descheduled host thread one
   * long gap */
  unsigned queries;
  double longest_query_us, longest_poll_gap_us;
} gsr_mailbox_event;
int gsr_mailbox_slow_path_last(gsr_mailbox_event* out);

const char* gsr_last_error(void);
int gsr_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GSRASTER_H_INCLUDED */
