/*
 * flow2d_c_abi.h -- the C boundary of the MI355X (gfx950) optical-flow hot path.
 *
 * What it replaces.  axruff/cuda-flow2d binds its host code to device code purely by C symbol
 * name: every operator class does cuModuleLoad("<exe>/kernels/<op>.ptx") + cuModuleGetFunction
 * and launches through cuLaunchKernel with a void* argument array (e.g.
 * src/cuda_operations/2d/cuda_operation_add_2d.cpp:50-55,96-103), and moves memory through the
 * CUDA driver API (src/utils/cuda_utils.cpp:26-105, src/optical_flow/optical_flow_2d.cpp:84-140).
 * This header is the drop-in for exactly that surface: device/context set-up, pitched plane
 * memory, one launcher per reference kernel, the solver's fixed-point loop, events.  Plain
 * pointers and sizes only; every function returns a flow2d_status (0 = ok) instead of printing.
 *
 * Conventions
 *  - A "plane" is a row-major fp32 image inside a pitched container: element (x, y) lives at
 *    base + y * pitch_bytes + 4 * x.  pitch_bytes is what DataSize3::pitch holds in the reference
 *    (src/data_types/data_structs.h:31-35); it must be a multiple of 16.  A pyramid level of
 *    w x h pixels occupies the top-left corner of a full-resolution container, as in the
 *    reference (`container_size` module constant, IND(X,Y) macro of every .cu file).
 *  - All launches go to the context's stream and return without synchronising.
 *  - Device pointers are raw HIP device addresses (void* / float*), caller-owned.
 *  - Not thread-safe per context; use one context per host thread / per GPU.
 *  - Arithmetic is IEEE fp32 in the reference's operation order with no fused multiply-add
 *    (kernels are built -ffp-contract=off), so results are bit-identical to the CPU oracle.
 */
#ifndef FLOW2D_C_ABI_H_
#define FLOW2D_C_ABI_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FLOW2D_API __attribute__((visibility("default")))

/* Additions that leave every existing entry as it was keep the version: flow2d_consistency_2d (forward-backward occlusion
 * masks), flow2d_flow_error_2d / flow2d_flow_error_workspace_bytes (error statistics against ground truth),
 * flow2d_interpolate_2d (occlusion-aware frame interpolation), flow2d_track_points_2d / flow2d_seed_points_2d /
 * flow2d_seed_points_workspace_bytes (dense point trajectories), flow2d_denoise_2d / flow2d_compose_flow_2d
 * (motion-compensated temporal denoising) and flow2d_global_motion_2d / flow2d_global_motion_workspace_bytes /
 * flow2d_global_flow_2d / flow2d_warp_global_2d (robust global motion and stabilisation), flow2d_segment_motion_2d /
 * flow2d_segment_motion_workspace_bytes (motion segmentation), flow2d_deformation_2d / flow2d_deformation_workspace_bytes
 * (strain, divergence and vorticity of a flow), flow2d_refine_flow_2d (edge-aware refinement of a flow), flow2d_correlate_2d /
 * flow2d_correlation_grid / flow2d_expand_nodes_2d (window correlation) and flow2d_prior_registration_2d (the first level of a
 * pyramid started from a prior flow) and flow2d_propagate_flow_2d (a flow carried along itself: the prior of a warm-started
 * sequence) and flow2d_fused_packed_launches (a test hook: which build of the strip kernel a launch took) and
 * flow2d_correlate_offset_2d / flow2d_validate_nodes_2d (multi-pass window correlation: the search around a predictor's
 * offset and the normalised median test between passes) and flow2d_subset_refine_2d (affine Gauss-Newton refinement of
 * correlation nodes) and flow2d_subset_refine_from_2d / flow2d_predict_nodes_2d (DIC over a sequence: the refinement started
 * from the previous step's deformation, and that start built from a step's result) and flow2d_node_strain_2d /
 * flow2d_node_strain_workspace_bytes (strain on the node grid from least-squares strain windows) and
 * flow2d_subset_refine_masked_2d (the refinement on a region of interest) and flow2d_bspline_prefilter_2d /
 * flow2d_subset_refine_spline_2d / flow2d_subset_refine2_spline_2d (the refinement with a cubic B-spline interpolation of the
 * deformed frame) and flow2d_context_set_planning_cus / flow2d_context_planning_cus (the CU count the launch planners plan
 * for) with the host-only diagnostics flow2d_fused_block_order_for_cus / flow2d_fused_plan_for_cus /
 * flow2d_stream_rows_for_cus (which plan a CU count gives) and flow2d_correlate_masked_2d / flow2d_validate_nodes_masked_2d (the
 * window search and the median test on a region of interest) and flow2d_node_strain_robust_2d /
 * flow2d_node_strain_robust_workspace_bytes (the strain windows as reweighted least squares, with diagnostic planes) and
 * flow2d_node_strain_weighted_2d / flow2d_node_strain_weighted_workspace_bytes (the strain windows weighted by the nodes' own
 * variances, with the standard deviations of the strain) were added under 1. */
#define FLOW2D_ABI_VERSION 1

typedef enum flow2d_status {
    FLOW2D_OK = 0,
    FLOW2D_ERR_INVALID_ARGUMENT = 1, /* null pointer, bad size, in == out, misaligned pitch */
    FLOW2D_ERR_NO_DEVICE = 2,        /* no usable HIP device / bad ordinal */
    FLOW2D_ERR_DEVICE = 3,           /* a HIP runtime call failed; see flow2d_last_error() */
    FLOW2D_ERR_OUT_OF_MEMORY = 4,
    FLOW2D_ERR_UNSUPPORTED = 5       /* e.g. median window not in {3,5,7}, Gaussian longer than 51 taps */
} flow2d_status;

/* Data term.  GREY, GRADIENT and LOG_DERIVATIVES are `enum class DataConstancy` Grey, Gradient and LogDerivatives
 * of the reference (src/data_types/data_structs.h:27), which selects solve_2d / solve_2d_grad / solve_2d_log with
 * them (src/cuda_operations/2d/cuda_operation_solve_2d.cpp:65-82); the numeric values here are the C-ABI's own
 * (the host layer maps the enum).  GRADIENT_UNTILED is an extra, opt-in mode with no counterpart in the reference: the gradient-constancy
 * tensor of solve_2d_grad with its second derivatives taken over the true neighbours (reflected at the image
 * border) instead of being cut at the reference's 16x8 launch tiles.  Results differ from
 * GRADIENT at tile edges by design. */
typedef enum flow2d_constancy {
    FLOW2D_CONSTANCY_GREY = 0,
    FLOW2D_CONSTANCY_GRADIENT = 1,
    FLOW2D_CONSTANCY_GRADIENT_UNTILED = 2,
    FLOW2D_CONSTANCY_LOG_DERIVATIVES = 3
} flow2d_constancy;

typedef struct flow2d_context flow2d_context; /* opaque: device ordinal + stream + scratch */

/* ---- library / errors ------------------------------------------------------------------ */
FLOW2D_API int flow2d_abi_version(void);
FLOW2D_API const char* flow2d_status_string(int status);
/* Text of the last failing HIP call on this thread ("" if none). */
FLOW2D_API const char* flow2d_last_error(void);

/* ---- device / context  (replaces InitCudaContextWithFirstAvailableDevice,
 *      src/utils/cuda_utils.cpp:26-62, and cuCtxDestroy at src/main.cpp:226) ----------------- */
FLOW2D_API int flow2d_device_count(int* count);
/* Hardware queues the HIP runtime deals this process's streams onto (GPU_MAX_HW_QUEUES; the runtime reads it once, at
 * its first call): the batched host path runs four lanes (streams) side by side and a lane that shares a queue waits
 * behind its neighbour.  flow2d_hw_queues returns the value the environment holds now (4 = the runtime's default when
 * unset or unparsable).  flow2d_request_hw_queues(n) asks for n queues: it sets the variable when the caller has not
 * and the process has not started the HIP runtime yet (FLOW2D_OK; also when the environment already grants n), and
 * reports FLOW2D_ERR_UNSUPPORTED -- with the reason in flow2d_last_error() -- when it came too late or the caller's own
 * value is smaller; nothing is changed then.  The host layer calls it before its first HIP call (InitDeviceContext).
 * No reference counterpart (one context, the NULL stream: src/utils/cuda_utils.cpp:43). */
FLOW2D_API int flow2d_hw_queues(void);
FLOW2D_API int flow2d_request_hw_queues(int queues);
FLOW2D_API int flow2d_context_create(int device_ordinal, flow2d_context** out_ctx);
/* Same, but launches on an existing hipStream_t owned by the caller (e.g. a PyTorch stream). */
FLOW2D_API int flow2d_context_create_on_stream(int device_ordinal, void* hip_stream, flow2d_context** out_ctx);
FLOW2D_API int flow2d_context_destroy(flow2d_context* ctx);
FLOW2D_API int flow2d_context_device(const flow2d_context* ctx, int* device_ordinal);
FLOW2D_API int flow2d_context_stream(const flow2d_context* ctx, void** hip_stream);
FLOW2D_API int flow2d_synchronize(flow2d_context* ctx); /* cuStreamSynchronize(NULL), cuda_operation_solve_2d.cpp:291 */
/* Lock-step batches of independent pairs (no reference counterpart): after flow2d_context_set_batch(ctx, count,
 * stride_bytes) every launcher, memset and device copy of this context acts on `count` instances of its planes,
 * instance b at plane pointer + b * stride_bytes (pairs stored one below the other in tall containers; stride a
 * multiple of 16).  One launch then holds the work of all instances (grid.z), so a level of a mid-size frame fills the
 * chip and the launch-bound coarse levels cost one launch per batch instead of one per pair.  count = 1 switches it
 * off (the default).  Results per instance are those of the unbatched call.  At most FLOW2D_BATCH_MAX instances (the
 * two-plane launches put 2 x count into grid.z).  count > 1 needs a non-zero stride that is a multiple of 16; count = 1
 * accepts any stride and ignores it.
 * Exceptions, which act as without a batch or refuse it: flow2d_copy_planes (its tables name every plane),
 * flow2d_copy_h2d_2d / flow2d_copy_d2h_2d (they move the one region asked for; a caller moves a whole group with
 * height = count x rows when the instances lie one below the other), flow2d_plane_alloc / flow2d_plane_free, and
 * flow2d_track_points_2d / flow2d_seed_points_2d, which return FLOW2D_ERR_UNSUPPORTED under a batch. */
#define FLOW2D_BATCH_MAX 32767
FLOW2D_API int flow2d_context_set_batch(flow2d_context* ctx, size_t count, size_t stride_bytes);
/* A hint, not a mode: lone != 0 says that the caller runs this context's launches alone on the device -- one pair after the
 * other, no other lane of the same job beside them (OpticalFlow2D::lone sets it; no reference counterpart, the reference has one
 * context and blocks after every launch, cuda_operation_solve_2d.cpp:291).  Strip launches of the solver that leave half the
 * device's wave slots empty then take the build of the strip kernel with packed arithmetic (a wave alone on its SIMD has nothing
 * to share issue turns with; the same IEEE operations, the same bits).  Default 0. */
FLOW2D_API int flow2d_context_set_lone(flow2d_context* ctx, int lone);
/* A hint, not a mode (no reference counterpart; added to ABI version 1 without changing any existing entry): the number of
 * compute units this context's launch planners plan for -- the strip plan of the fused solver (strip heights, launch order,
 * whether a lock-step group shares a launch, and the size up to which a lone context takes the packed build) and the rows per
 * strip of the streaming Gaussian and median kernels.  Every value gives the same bytes; only the launch geometry changes.  A
 * context starts with its device's own count; cus = 0 goes back to it, 1 ... FLOW2D_PLANNING_CUS_MAX is taken as given (it need
 * not be a count any device has: a test runs the plans of a small or partitioned device on whatever device it finds).  A null
 * context or any other value is FLOW2D_ERR_INVALID_ARGUMENT and leaves the count as it was.  A plan is fixed when a launch is
 * queued, so a recorded graph (flow2d_capture_begin) keeps the plans it was captured with whatever is set when it is replayed.
 * flow2d_context_planning_cus reads the count the planners use now.  Neither call touches the device. */
#define FLOW2D_PLANNING_CUS_MAX 4096
FLOW2D_API int flow2d_context_set_planning_cus(flow2d_context* ctx, int cus);
FLOW2D_API int flow2d_context_planning_cus(const flow2d_context* ctx, int* cus);
/* cuMemGetInfo, optical_flow_2d.cpp:91 */
FLOW2D_API int flow2d_mem_info(flow2d_context* ctx, size_t* free_bytes, size_t* total_bytes);
FLOW2D_API int flow2d_device_name(flow2d_context* ctx, char* buf, size_t buf_len);

/* ---- pitched plane memory  (replaces cuMemAllocPitch / cuMemFree / cuMemsetD2D8 / cuMemcpy2D /
 *      cuMemcpyDtoD: optical_flow_2d.cpp:114-133,309-312,574-577; cuda_utils.cpp:66-105;
 *      cuda_operation_median_2d.cpp:100-104) -------------------------------------------------- */
/* Row pitch this library uses for a plane of `width` floats (multiple of 256 bytes). */
FLOW2D_API size_t flow2d_plane_pitch_bytes(size_t width);
FLOW2D_API int flow2d_plane_alloc(flow2d_context* ctx, size_t width, size_t height, void** out_dev_ptr,
                                  size_t* out_pitch_bytes);
FLOW2D_API int flow2d_plane_free(flow2d_context* ctx, void* dev_ptr);
FLOW2D_API int flow2d_memset_2d(flow2d_context* ctx, void* dev_ptr, size_t pitch_bytes, int byte_value,
                                size_t width_bytes, size_t height);
FLOW2D_API int flow2d_copy_h2d_2d(flow2d_context* ctx, void* dst_dev, size_t dst_pitch_bytes, const void* src_host,
                                  size_t src_pitch_bytes, size_t width_bytes, size_t height);
FLOW2D_API int flow2d_copy_d2h_2d(flow2d_context* ctx, void* dst_host, size_t dst_pitch_bytes, const void* src_dev,
                                  size_t src_pitch_bytes, size_t width_bytes, size_t height);
FLOW2D_API int flow2d_copy_d2d(flow2d_context* ctx, void* dst_dev, const void* src_dev, size_t bytes);

/* `count` (at most FLOW2D_COPY_PLANES_MAX) independent planes of one geometry copied by ONE launch on the context's stream:
 * plane i from src_planes[i] to dst_planes[i] (width floats x height rows, both of pitch_bytes).  This is how a lock-step
 * group gathers pairs that live in containers of their own into its tall staging containers and hands the flows back
 * (OpticalFlow2D::ComputeFlowGroupDevice): two launches per group instead of 4 x count cuMemcpyDtoD calls.  Not subject
 * to flow2d_context_set_batch (the tables name every plane). */
#define FLOW2D_COPY_PLANES_MAX 64
FLOW2D_API int flow2d_copy_planes(flow2d_context* ctx, size_t count, const void* const* src_planes,
                                  void* const* dst_planes, size_t pitch_bytes, size_t width, size_t height);

/* ---- page-locked host memory  (replaces cuMemAllocHost / cuMemFreeHost, the reference's ALLOCATE_PINNED_MEMORY
 *      option: src/data_types/data2d.cpp:34,60-61,80-82) --------------------------------------------------------
 * flow2d_copy_h2d_2d / flow2d_copy_d2h_2d are asynchronous on the context's stream; from and to pageable memory the
 * runtime stages them through its own bounce buffers and the call returns when the bytes have left the caller's
 * buffer (about 20 GB/s).  From and to memory allocated here the copy is one DMA transfer at the PCIe rate, returns at
 * once and overlaps kernels of other streams: the host buffer must stay untouched until the stream has passed the
 * copy (flow2d_synchronize, or an event recorded behind it).  ctx may be NULL (the calling thread's current device). */
FLOW2D_API int flow2d_host_alloc(flow2d_context* ctx, size_t bytes, void** out_host_ptr);
FLOW2D_API int flow2d_host_free(flow2d_context* ctx, void* host_ptr);

/* ---- events  (replaces cuEventCreate/Record/Synchronize/ElapsedTime/Destroy,
 *      optical_flow_2d.cpp:173-179,548-557; cuda_operation_solve_2d.cpp:214-220,302-313) ------- */
FLOW2D_API int flow2d_event_create(flow2d_context* ctx, void** out_event);
FLOW2D_API int flow2d_event_record(flow2d_context* ctx, void* event);
FLOW2D_API int flow2d_event_synchronize(flow2d_context* ctx, void* event);
FLOW2D_API int flow2d_event_elapsed_ms(flow2d_context* ctx, void* start_event, void* stop_event, float* out_ms);
FLOW2D_API int flow2d_event_destroy(flow2d_context* ctx, void* event);
/* Everything queued on `ctx` after this call waits until the work recorded into `event` (by flow2d_event_record on any
 * context of the same device) has finished; the host does not wait.  An event never recorded counts as finished.  This
 * is what chains work on several contexts -- copy streams, compute streams -- into a pipeline (no reference
 * counterpart: one NULL stream, host-synchronous copies, src/utils/cuda_utils.cpp:66-105). */
FLOW2D_API int flow2d_stream_wait_event(flow2d_context* ctx, void* event);

/* ---- stream capture (no counterpart in the reference, which launches eagerly and blocks after every
 *      sweep).  Everything queued on the context between begin and end is recorded into a HIP graph
 *      instead of being executed; flow2d_graph_launch replays it with one host call.  Used by the host
 *      layer to replay a whole pyramid (several hundred launches) for repeated pairs of one size.
 *      Only stream-ordered calls are legal while capturing (no alloc/free/synchronise/event query). --- */
FLOW2D_API int flow2d_capture_begin(flow2d_context* ctx);
FLOW2D_API int flow2d_capture_end(flow2d_context* ctx, void** out_graph_exec);
FLOW2D_API int flow2d_graph_launch(flow2d_context* ctx, void* graph_exec);
FLOW2D_API int flow2d_graph_destroy(flow2d_context* ctx, void* graph_exec);

/* ---- kernel launchers: one per `extern "C" __global__` symbol of src/kernels/ -------------- */

/* The core entries: the launchers of the reference's kernels and their fused forms, the hot path of the flow --
 *   flow2d_add_2d, flow2d_add_2d_pair, flow2d_copy_planes, flow2d_convolution_rows, flow2d_convolution_columns,
 *   flow2d_gaussian_blur, flow2d_median_2d, flow2d_median_2d_pair, flow2d_add_median_2d_pair, flow2d_add_median_2d_pair_half,
 *   flow2d_registration_2d, flow2d_upsample_registration_2d, flow2d_upsample_registration_half_2d, flow2d_resample_x,
 *   flow2d_resample_y, flow2d_resample_x_pair, flow2d_resample_y_pair, flow2d_resample_xy_pair, flow2d_resample_x_levels,
 *   flow2d_resample_y_levels, flow2d_resample_xy_levels, flow2d_compute_phi_ksi, flow2d_solve_2d, flow2d_solve_2d_grad,
 *   flow2d_solve_2d_grad_untiled, flow2d_solve_2d_log, flow2d_solve_2d_sor, flow2d_solve_level.
 * Their alias rule, stated once.  A plane argument of `rows` rows stands for the bytes [p, p + rows * pitch_bytes) -- with
 * flow2d_context_set_batch for those bytes of every instance, [p + b * stride, p + b * stride + rows * pitch_bytes), b < count --
 * and pitch_bytes covers every byte a kernel may read or write for the plane: a kernel reads a row beyond its width only inside
 * the row's pitch (the second column of a pair at width 1, the tail of a 16-byte load), never into another row's bytes that the
 * call does not own, and writes inside width x rows only.  rows is the height the entry is given for the plane (in_height for
 * the smaller input of a resample or an up-sampling, (height + 1) / 2 for a half-size base flow, the rows between the first and
 * the last region of a plane written in regions; flow_du / flow_dv of flow2d_solve_level count with container_height rows where
 * the per-sweep path zeroes them).  One exception: the input of flow2d_resample_y / flow2d_resample_y_pair may be a column segment
 * of a packed plane, `packed + column_offsets[l]`; its last row ends with the segment (out_width floats, rounded up to 16 bytes).
 * No written range may share a byte with a read range, with another written range or with another instance of itself:
 * FLOW2D_ERR_INVALID_ARGUMENT before anything is launched or copied, whatever the base pointers are -- an output that starts one
 * row, one instance or sixteen bytes into an input is refused like one on the input's base.  The test is exact per instance, not
 * a test of the hulls: groups laid out A0 B0 A1 B1 (stride = two planes) share no byte and pass.  Read planes may meet each
 * other freely.  In place, on exactly the same base and only there: operand_0 of flow2d_add_2d / flow2d_add_2d_pair is read and
 * written, and its own operand_1 may be that same plane; flow2d_solve_2d_sor relaxes flow_du / flow_dv in place.  No other
 * argument of a core entry may be a plane the call writes.  flow2d_copy_planes applies the rule to all its destinations against
 * all its sources and each other, without a batch. */

/* add_2d (src/kernels/add_2d.cu:33-46): operand_0 += operand_1 on w x h. */
FLOW2D_API int flow2d_add_2d(flow2d_context* ctx, float* operand_0, const float* operand_1, size_t width,
                             size_t height, size_t pitch_bytes);

/* Host-side Gaussian taps, CudaOperationConvolution2D::ComputeGaussianKernel(sigma, 3, 1.0)
 * (src/cuda_operations/2d/cuda_operation_convolution_2d.cpp:83-112).  taps must hold 51 floats
 * (MAX_KERNEL_LENGTH, convolution_2d.cu:49); writes 2*radius+1 of them. */
FLOW2D_API int flow2d_gaussian_kernel(float sigma, float* taps, int* out_radius);

/* convolutionRowsKernel / convolutionColumnsKernel (src/kernels/convolution_2d.cu:74-168,181-261).
 * `taps` is a HOST array of 2*radius+1 floats (the reference uploads it to the module constant
 * c_Kernel, cuda_operation_convolution_2d.cpp:163-164).  Zero padding outside the image. */
FLOW2D_API int flow2d_convolution_rows(flow2d_context* ctx, float* dst, const float* src, size_t width, size_t height,
                                       size_t pitch_bytes, const float* taps, int radius);
FLOW2D_API int flow2d_convolution_columns(flow2d_context* ctx, float* dst, const float* src, size_t width,
                                          size_t height, size_t pitch_bytes, const float* taps, int radius);

/* Both passes of the separable Gaussian in one launch (rows pass into LDS, columns pass out of it): the
 * result equals flow2d_convolution_rows into a temp followed by flow2d_convolution_columns bit for bit,
 * with half the DRAM traffic.  Replaces the pair of launches of CudaOperationConvolution2D::Execute
 * (cuda_operation_convolution_2d.cpp:169-175); no temp plane needed. */
FLOW2D_API int flow2d_gaussian_blur(flow2d_context* ctx, float* dst, const float* src, size_t width, size_t height,
                                    size_t pitch_bytes, const float* taps, int radius);

/* median_2d (src/kernels/median_2d.cu:87-299): `window` is the window width (3, 5 or 7; the
 * reference calls it "radius"), mirror borders. */
FLOW2D_API int flow2d_median_2d(flow2d_context* ctx, const float* input, size_t width, size_t height,
                                size_t pitch_bytes, size_t window, float* output);

/* registration_2d (src/kernels/registration_2d.cu:34-73): backward bilinear warp of frame_1. */
FLOW2D_API int flow2d_registration_2d(flow2d_context* ctx, const float* frame_0, const float* frame_1,
                                      const float* flow_u, const float* flow_v, size_t width, size_t height,
                                      size_t pitch_bytes, float hx, float hy, float* output);

/* Forward-backward consistency check (Sundaram, Brox & Keutzer, ECCV 2010; no reference counterpart; added to ABI version 1
 * without changing any existing entry).  (flow_u, flow_v): the flow of frame 0 to frame 1; (back_u, back_v): the flow of
 * frame 1 to frame 0.  For every pixel (x, y), 0 <= x < width, 0 <= y < height, `mask` gets 1.0f where the pair is
 * inconsistent -- occluded, leaving the frame, or NaN -- and 0.0f elsewhere, by exactly these fp32 operations:
 *   xf = x + u0, yf = y + v0                          (u0 = flow_u[p], v0 = flow_v[p])
 *   not (0 <= xf <= width - 1 and 0 <= yf <= height - 1)  -> 1          (a NaN lands here)
 *   xi = floor(xf), yi = floor(yf), dx = xf - xi, dy = yf - yi, x1 = min(width - 1, xi + 1), y1 = min(height - 1, yi + 1)
 *   S(P) = (1-dx)*(1-dy)*P[yi,xi] + dx*(1-dy)*P[yi,x1] + (1-dx)*dy*P[y1,xi] + dx*dy*P[y1,x1]  (left to right: the bilinear
 *          sample of flow2d_registration_2d)
 *   bu = S(back_u), bv = S(back_v), eu = u0 + bu, ev = v0 + bv
 *   mask = (eu*eu + ev*ev <= alpha1 * ((u0*u0 + v0*v0) + (bu*bu + bv*bv)) + alpha2) ? 0 : 1   (a NaN sample -> 1)
 * The paper's values are alpha1 = 0.01, alpha2 = 0.5.  FLOW2D_ERR_INVALID_ARGUMENT for a null plane, a zero size, a negative or
 * non-finite alpha, or a `mask` whose bytes [mask, mask + height * pitch_bytes) -- over every instance of a batch -- overlap
 * those of any input plane.  Honours flow2d_context_set_batch.  Pitch at least 4 floats (the bilinear sample reads column pairs;
 * at width 1 the second column is row padding and never selected). */
FLOW2D_API int flow2d_consistency_2d(flow2d_context* ctx, const float* flow_u, const float* flow_v, const float* back_u,
                                     const float* back_v, size_t width, size_t height, size_t pitch_bytes, float alpha1,
                                     float alpha2, float* mask);

/* Occlusion-aware frame interpolation from a bidirectional flow (no reference counterpart; added to ABI version 1 without
 * changing any existing entry).  (flow_u, flow_v): the flow of frame_0 to frame_1; (back_u, back_v): the flow of frame_1 to
 * frame_0; occlusion_0 / occlusion_1: the occlusion masks of frame_0 / frame_1 (1 = no match in the other frame, as
 * flow2d_consistency_2d writes them), each may be NULL on its own.  `output` gets the frame at time t, 0 <= t <= 1, by exactly
 * these fp32 operations, in this order, for every pixel x = (x, y):
 *   S(P, p)   the bilinear sample of flow2d_consistency_2d at p, where p is first replaced by x when either coordinate is not
 *             finite and then clamped to [0, width - 1] x [0, height - 1]; both components of a flow are sampled at one p
 *   side 0    p_0 = x;  p_k = x - t * S(flow, p_{k-1}) for k = 1 .. K (K = iterations; per component);
 *             r = x - t * S(flow, p_K) - p_K;
 *             ok0 = p_K finite and inside [0, width - 1] x [0, height - 1] and r.x*r.x + r.y*r.y <= max_residual*max_residual;
 *             a0 = S(frame_0, p_K)
 *   side 1    the same with (back_u, back_v) and s = 1 - t in place of t: q_K, ok1, a1 = S(frame_1, q_K)
 *   masks     c0 = ok0 ? S(occlusion_0, p_K) : 0 (0 when occlusion_0 is NULL); then if (!(c0 <= 1)) c0 = 1;
 *             if (!(c0 >= 0)) c0 = 0 (a NaN counts as occluded); c1 likewise with occlusion_1 at q_K
 *   weights   v0 = ok0 * (1 - c0), v1 = ok1 * (1 - c1)   (ok as 0.0f / 1.0f);
 *             v0 + v1 > 0:  w0 = s * v0, w1 = t * v1   (content seen in both frames wins over content seen in one)
 *             otherwise:    w0 = s * ok0, w1 = t * ok1
 *   output    w0 + w1 > 0:  (w0*a0 + w1*a1) / (w0 + w1)   (correctly rounded division)
 *             otherwise:    s*a0 + t*a1
 * With finite flows, no masks and frames without negative zeros the output is frame_0 bit for bit at t = 0 and frame_1 at t = 1.
 * FLOW2D_ERR_INVALID_ARGUMENT for a null required plane, a zero size, a bad pitch (a multiple of 16 bytes, at least 4 floats:
 * the sample reads column pairs), a t that is not finite or outside [0, 1], iterations outside [1, 16], a negative or
 * non-finite max_residual, or an `output` whose bytes [output, output + height * pitch_bytes) -- over every instance of a
 * batch -- overlap those of any input plane.  Honours flow2d_context_set_batch.  One launch, no allocation, no
 * synchronisation (graph-capturable). */
FLOW2D_API int flow2d_interpolate_2d(flow2d_context* ctx, const float* frame_0, const float* frame_1, const float* flow_u,
                                     const float* flow_v, const float* back_u, const float* back_v, const float* occlusion_0,
                                     const float* occlusion_1, size_t width, size_t height, size_t pitch_bytes, float t,
                                     int iterations, float max_residual, float* output);

/* Dense point trajectories (Sundaram, Brox & Keutzer, ECCV 2010; no reference counterpart; added to ABI version 1 without
 * changing any existing entry).  A track table is `capacity` floats of x and `capacity` floats of y (device memory); slot i
 * holds a track's position in one frame, NaN where the track has not started or has ended.  `count` (DEVICE memory, read on
 * the device, never by the host) is the number of slots in use.
 *
 * flow2d_track_points_2d advances a table by one flow step.  (flow_u, flow_v): the flow of frame k to frame k+1; (back_u,
 * back_v): the flow of frame k+1 to frame k, or both NULL (no forward-backward check).  For every slot i < capacity, with
 * n = *count, the first of these that applies gives `reason[i]` (when `reason` is not NULL), in fp32 and in this order:
 *   1 INACTIVE         i >= n, or x[i] or y[i] is not finite
 *   3 LEFT_FRAME       p = (x[i], y[i]) outside [0, width - 1] x [0, height - 1]
 *                      u0 = S(flow_u, p), v0 = S(flow_v, p)   (S: the bilinear sample of flow2d_consistency_2d, same order)
 *   2 MOTION_BOUNDARY  only when check_boundaries != 0:  (ix, iy) = ((int)floorf(px + 0.5f), (int)floorf(py + 0.5f));
 *                      ux = 0.5f * (U[iy][min(ix+1, width-1)] - U[iy][max(ix-1, 0)]),
 *                      uy = 0.5f * (U[min(iy+1, height-1)][ix] - U[max(iy-1, 0)][ix]), vx, vy likewise on V;
 *                      g = (ux*ux + uy*uy) + (vx*vx + vy*vy);  !(g <= beta1 * (u0*u0 + v0*v0) + beta2)  (a NaN lands here;
 *                      the paper's values are beta1 = 0.01, beta2 = 0.002)
 *                      q = (px + u0, py + v0)
 *   4 OCCLUDED         q not finite
 *   3 LEFT_FRAME       q outside the frame
 *   4 OCCLUDED         only with back planes: bu = S(back_u, q), bv = S(back_v, q), eu = u0 + bu, ev = v0 + bv;
 *                      !(eu*eu + ev*ev <= alpha1 * ((u0*u0 + v0*v0) + (bu*bu + bv*bv)) + alpha2)  (the inequality of
 *                      flow2d_consistency_2d at the track's sub-pixel position)
 *   0 ALIVE            out_x[i] = qx, out_y[i] = qy
 * Whenever the reason is not 0, out_x[i] = out_y[i] = NaN.  Every slot below `capacity` is written.
 * FLOW2D_ERR_INVALID_ARGUMENT for a null required pointer or only one back plane, a zero size or capacity, a bad pitch (the
 * rule of flow2d_interpolate_2d), a negative or non-finite alpha or beta, or outputs (out_x, out_y, reason) whose bytes overlap
 * those of any input (planes: height * pitch_bytes; tables: 4 * capacity; count: 8) or each other.
 * FLOW2D_ERR_UNSUPPORTED under a lock-step batch (flow2d_context_set_batch count above 1) and for capacity >= 2^40.  Slot
 * offsets are 64-bit.  One launch, no allocation, no synchronisation (graph-capturable). */
typedef enum flow2d_track_reason {
    FLOW2D_TRACK_ALIVE = 0,
    FLOW2D_TRACK_INACTIVE = 1,
    FLOW2D_TRACK_MOTION_BOUNDARY = 2,
    FLOW2D_TRACK_LEFT_FRAME = 3,
    FLOW2D_TRACK_OCCLUDED = 4
} flow2d_track_reason;
FLOW2D_API int flow2d_track_points_2d(flow2d_context* ctx, const float* flow_u, const float* flow_v, const float* back_u,
                                      const float* back_v, size_t width, size_t height, size_t pitch_bytes, const float* x,
                                      const float* y, const unsigned long long* count /* device */, size_t capacity,
                                      float alpha1, float alpha2, int check_boundaries, float beta1, float beta2, float* out_x,
                                      float* out_y, unsigned char* reason /* may be NULL */);

/* flow2d_seed_points_2d appends new tracks in uncovered, textured cells of `frame`.  With s = spacing:
 *   cells          ceil(width / s) x ceil(height / s); cell (i, j) holds the pixels [i*s, (i+1)*s) x [j*s, (j+1)*s); its seed
 *                  pixel is (min(i*s + s/2, width - 1), min(j*s + s/2, height - 1)) (integer division; s = 1: every pixel)
 *   covered        some slot k < *count has finite x[k], y[k] inside [0, width - 1] x [0, height - 1] with
 *                  ((int)floorf(x[k]) / s, (int)floorf(y[k]) / s) == (i, j)
 *   seedable       min_eigenvalue == 0, or lambda_min >= min_eigenvalue at the seed pixel, where
 *                  gx = 0.5f * (F[y][min(x+1, width-1)] - F[y][max(x-1, 0)]), gy likewise along y (clamped neighbours);
 *                  a = sum gx*gx, b = sum gx*gy, c = sum gy*gy over the 5x5 window around the seed pixel, coordinates
 *                  clamped to the frame (edge-replicated), each sum from 0.0f in row-major order;
 *                  lambda_min = 0.5f*(a + c) - sqrtf(0.25f*(a - c)*(a - c) + b*b)   (correctly rounded sqrtf)
 * Every uncovered, seedable cell, in row-major cell order, gets slot *count + m (m = 0, 1, ...) with x, y = its seed pixel,
 * until `capacity` is reached; *count grows by the number written and *dropped (when not NULL, DEVICE memory) gets the number
 * of cells that did not fit.  Slots below the old *count are not touched.  Deterministic: the slot of a seed depends only on
 * the cell order (per-block counts, a scan in block order, the writes; no atomics), so repeats and graph replays write the
 * same bytes.  *count == 0 is the initial seeding of a sequence.  Five launches into the caller's `workspace` (16-byte
 * aligned, at least flow2d_seed_points_workspace_bytes(width, height, spacing) bytes), no allocation, no synchronisation
 * (graph-capturable).  min_eigenvalue is in the units of unnormalised sums of squared grey-level gradients.
 * FLOW2D_ERR_INVALID_ARGUMENT for a null required pointer, a zero size, spacing or capacity, a bad pitch, a negative or
 * non-finite min_eigenvalue, a misaligned count / dropped / workspace, a workspace too small, or overlapping bytes among
 * frame, x, y, count, dropped and the workspace.  FLOW2D_ERR_UNSUPPORTED under a lock-step batch, for capacity >= 2^40 and
 * for 2^32 cells or more. */
FLOW2D_API size_t flow2d_seed_points_workspace_bytes(size_t width, size_t height, size_t spacing);
FLOW2D_API int flow2d_seed_points_2d(flow2d_context* ctx, const float* frame, size_t width, size_t height, size_t pitch_bytes,
                                     size_t spacing, float min_eigenvalue, float* x, float* y,
                                     unsigned long long* count /* device, read and updated */, size_t capacity,
                                     unsigned long long* dropped /* device, may be NULL */, void* workspace,
                                     size_t workspace_bytes);

/* Motion-compensated temporal denoising (no reference counterpart; added to ABI version 1 without changing any existing
 * entry).  flow2d_denoise_2d fuses `centre` with N = neighbour_count (1 .. FLOW2D_DENOISE_MAX_NEIGHBOURS) neighbour frames in one
 * launch.  frames, flows_u, flows_v and occlusions are HOST arrays of N device planes: (flows_u[n], flows_v[n]) is the flow from
 * the centre frame to frames[n] on the centre's grid; occlusions[n] is the occlusion mask of that flow on the centre's grid (1 =
 * no match in frames[n], as flow2d_consistency_2d writes it) -- the array, or any entry of it, may be NULL (nothing occluded).
 * For every pixel x = (x, y), with c = centre[x], by exactly these fp32 operations, in this order:
 *   num = c;  den = 1
 *   for n = 0 .. N - 1:
 *     q   = x + (flows_u[n][x], flows_v[n][x])                                  (per component)
 *     ok  = 0 <= q.x <= width - 1 and 0 <= q.y <= height - 1                    (a NaN or an infinity fails)
 *     s   = S(frames[n], ok ? q : x)         (S: the bilinear sample of flow2d_consistency_2d, same order; every read stays
 *                                            inside the plane)
 *     m   = occlusions[n] ? occlusions[n][x] : 0;  if (!(m <= 1)) m = 1;  if (!(m >= 0)) m = 0    (a NaN counts as occluded)
 *     d   = s - c
 *     g   = range_sigma == 0 ? 1 : (range_sigma*range_sigma) / (range_sigma*range_sigma + d*d)    (correctly rounded division)
 *     wgt = ok ? (1 - m) * g : 0;   t = wgt * s;   if t is not finite: wgt = 0, t = 0   (a NaN or infinite sample, a NaN weight)
 *     num = num + t;  den = den + wgt                                            (separate multiply and add)
 *   output[x] = num / den   (correctly rounded division);   weight_sum[x] = den   (when weight_sum is not NULL)
 * range_sigma is in grey levels; 0 switches the photometric weight g off.  den is at least 1 and at most N + 1; where every
 * neighbour is occluded, has a NaN flow or points out of the frame, output is the centre bit for bit (frames without negative
 * zeros).  A NaN flow is what flow2d_compose_flow_2d writes for a broken chain: such a neighbour contributes nothing.
 * FLOW2D_ERR_INVALID_ARGUMENT for neighbour_count outside 1 .. 8, a null array or required plane, a zero size, a bad pitch (the
 * rule of flow2d_consistency_2d), a negative or non-finite range_sigma, or an `output` / `weight_sum` whose bytes [p, p + height *
 * pitch_bytes) -- over every instance of a batch -- overlap those of any input plane or of each other.  Honours
 * flow2d_context_set_batch (the pointers are those of instance 0).  One launch, no allocation, no synchronisation
 * (graph-capturable). */
#define FLOW2D_DENOISE_MAX_NEIGHBOURS 8
FLOW2D_API int flow2d_denoise_2d(flow2d_context* ctx, const float* centre, size_t neighbour_count, const float* const* frames,
                                 const float* const* flows_u, const float* const* flows_v,
                                 const float* const* occlusions /* may be NULL, and so may its entries */, size_t width,
                                 size_t height, size_t pitch_bytes, float range_sigma, float* output,
                                 float* weight_sum /* may be NULL */);

/* Flow concatenation: (ab_u, ab_v), the flow of frame a to frame b on a's grid, followed by (bc_u, bc_v), the flow of frame b to
 * frame c on b's grid, gives the flow of a to c on a's grid -- how flow2d_denoise_2d reaches neighbours further than one frame
 * away, and the accumulated displacement against a reference frame.  For every pixel x, in fp32:
 *   q = x + (ab_u[x], ab_v[x]);  ok = 0 <= q.x <= width - 1 and 0 <= q.y <= height - 1     (a NaN or an infinity fails)
 *   out_u[x] = ok ? ab_u[x] + S(bc_u, q) : NaN,  out_v likewise   (S as above; every NaN written is the quiet NaN 0x7fc00000)
 *   out_mask[x] = (!ok || !(mask_ab[x] == 0) || !(S(mask_bc, q) <= 0)) ? 1 : 0
 * mask_ab (a's grid, the mask of a -> b), mask_bc (b's grid, the mask of b -> c) and out_mask are optional: a NULL input mask
 * counts as 0 everywhere, and without out_mask no mask is read.  FLOW2D_ERR_INVALID_ARGUMENT for a null required plane, a zero
 * size, a bad pitch (the rule of flow2d_consistency_2d), or a written plane whose bytes -- over every instance of a batch --
 * overlap those of any input plane or of another written one.  Honours flow2d_context_set_batch.  One launch, no allocation, no
 * synchronisation (graph-capturable). */
FLOW2D_API int flow2d_compose_flow_2d(flow2d_context* ctx, const float* ab_u, const float* ab_v, const float* bc_u,
                                      const float* bc_v, const float* mask_ab /* may be NULL */,
                                      const float* mask_bc /* may be NULL */, size_t width, size_t height, size_t pitch_bytes,
                                      float* out_u, float* out_v, float* out_mask /* may be NULL */);

/* Error of a flow estimate against ground truth (Barron et al. 1994, Baker et al. 2011 -- Middlebury --, Menze & Geiger 2015 --
 * KITTI --; no reference counterpart; added to ABI version 1 without changing any existing entry).
 * For every pixel p, 0 <= x < width, 0 <= y < height, with u = flow_u[p], v = flow_v[p], gu = gt_u[p], gv = gt_v[p], all fp32:
 *   valid ground truth      |gu| <= 1e9 and |gv| <= 1e9 (finite; larger values are Middlebury's UNKNOWN_FLOW_THRESH)
 *                           otherwise counted in invalid_ground_truth and nothing else
 *   non-finite estimate     u or v infinite or NaN at a valid pixel: counted in nonfinite_estimate and nothing else
 *   du = u - gu, dv = v - gv, epe = sqrtf(du*du + dv*dv)                              (correctly rounded sqrtf)
 *   cx = v - gv, cy = gu - u, cz = u*gv - v*gu, cross = sqrtf((cx*cx + cy*cy) + cz*cz), dot = (u*gu + v*gv) + 1
 *   ae = atan2f(cross, dot) * 57.29577951308232f      (degrees between (u, v, 1) and (gu, gv, 1): the atan2 form, which keeps
 *                                                     its precision at small angles; within 1e-4 degrees of the exact angle
 *                                                     for |flow| <= 1e3; meaningless -- 90 degrees or NaN -- once the
 *                                                     products overflow, for estimates beyond ~1e19)
 *   gmag = sqrtf(gu*gu + gv*gv)
 *   class                   occ where occlusion != NULL and occlusion[p] != 0 (NaN included: what flow2d_consistency_2d
 *                           writes, and what a ground-truth occlusion map holds), noc elsewhere; all = noc + occ
 * Per class: count; above[k] = pixels with epe > 0.5, 1, 2, 3 (Middlebury R0.5 / R1 / R2 and the 3-px rate); fl = pixels with
 * epe > 3 and epe > 0.05f * gmag (KITTI Fl); sum_epe, sum_epe_sq (= sum of (double)epe * (double)epe) and sum_ae in double;
 * max_epe (0 for an empty class).  An infinite epe (a finite estimate whose du*du overflows) enters the sums as inf.
 * Outputs: `epe` / `ae` (either may be NULL) get the per-pixel values, NaN where the pixel is invalid or the estimate
 * non-finite; stats[b] (DEVICE memory) gets the record of instance b of a lock-step batch.
 * Deterministic: counts are exact and the double sums run in a fixed order that depends only on (width, height), so repeated
 * calls and an instance of a batch alone or in its group give the same bytes.  No allocation, no synchronisation: two launches
 * on the context's stream (graph-capturable) into the caller's `workspace`, which holds at least
 * flow2d_flow_error_workspace_bytes(width, height, instances) bytes (16-byte aligned; instances = the batch count).
 * FLOW2D_ERR_INVALID_ARGUMENT for a null required plane, a zero size, a bad pitch, a null or misaligned `stats` or
 * `workspace`, a workspace too small, or an `epe` / `ae` whose bytes [p, p + height * pitch_bytes) -- over every instance of a
 * batch -- overlap those of any input plane or of each other, or those of `stats` or the workspace. */
typedef struct flow2d_flow_error_class {
    unsigned long long count;
    unsigned long long above[4]; /* epe > 0.5, 1, 2, 3 */
    unsigned long long fl;       /* epe > 3 and epe > 0.05 |gt| */
    double sum_epe;
    double sum_epe_sq;
    double sum_ae;               /* degrees */
    double max_epe;
} flow2d_flow_error_class;

typedef struct flow2d_flow_error_stats {
    flow2d_flow_error_class all, noc, occ;
    unsigned long long invalid_ground_truth;
    unsigned long long nonfinite_estimate;
} flow2d_flow_error_stats;

#define FLOW2D_FLOW_ERROR_STATS_BYTES 256
#ifdef __cplusplus
static_assert(sizeof(flow2d_flow_error_stats) == FLOW2D_FLOW_ERROR_STATS_BYTES, "flow2d_flow_error_stats layout");
#else
_Static_assert(sizeof(flow2d_flow_error_stats) == FLOW2D_FLOW_ERROR_STATS_BYTES, "flow2d_flow_error_stats layout");
#endif

/* Workspace bytes flow2d_flow_error_2d needs for `instances` lock-step instances of a width x height pair (0 for a zero size).
 * Host logic only, needs no device. */
FLOW2D_API size_t flow2d_flow_error_workspace_bytes(size_t width, size_t height, size_t instances);
FLOW2D_API int flow2d_flow_error_2d(flow2d_context* ctx, const float* flow_u, const float* flow_v, const float* gt_u,
                                    const float* gt_v, const float* occlusion, size_t width, size_t height, size_t pitch_bytes,
                                    float* epe, float* ae, flow2d_flow_error_stats* stats, void* workspace,
                                    size_t workspace_bytes);

/* Robust global motion of a flow field, and what it is good for (no reference counterpart; added to ABI version 1 without
 * changing any existing entry): the parametric motion of the whole frame fitted to a flow by iteratively reweighted least
 * squares (flow2d_global_motion_2d), that model as planes with the residual flow and the inlier map (flow2d_global_flow_2d),
 * and a frame resampled along a model (flow2d_warp_global_2d: stabilisation).
 *
 * The model, in coordinates centred on the frame, xc = x - (width - 1) / 2, yc = y - (height - 1) / 2:
 *   mu(x) = (p0 + p1*xc) + p2*yc,   mv(x) = (p3 + p4*xc) + p5*yc
 * All arithmetic of the three entries is IEEE double, every operation rounded on its own (no fused multiply-add), in the order
 * written here; x, y, width - 1 and height - 1 convert exactly and the halves are exact.
 *
 * flow2d_global_motion_2d fits `model` to (flow_u, flow_v).  Per pixel, with u = flow_u[p], v = flow_v[p] (fp32, converted):
 *   valid = |u| <= 1e9 and |v| <= 1e9                 (finite: the rule of flow2d_flow_error_2d's ground truth)
 *   m     = mask ? mask[p] : 0;  if (!(m <= 1)) m = 1;  if (!(m >= 0)) m = 0      (fp32, the clamp of flow2d_denoise_2d: NaN = 1;
 *           `mask` is 1 where the vector is to be left out, as flow2d_consistency_2d writes it)
 *   b     = valid ? 1 - m : 0   (1 - m in fp32, then converted);   an invalid pixel takes part with u = v = 0 and w = 0
 *   pass 0:                       w = b
 *   pass k = 1 .. iterations, only when sigma > 0, with the parameters p of pass k - 1:
 *                                 du = u - ((p0 + p1*xc) + p2*yc),  dv = v - ((p3 + p4*xc) + p5*yc),
 *                                 w = b * (s2 / (s2 + (du*du + dv*dv))),   s2 = sigma*sigma
 *   (the rational weight of flow2d_denoise_2d; sigma in pixels; with sigma == 0 only pass 0 runs: plain least squares)
 * Every pass forms twelve sums over the frame, with wx = w*xc, wy = w*yc:
 *   S0 = sum w, Sx = sum wx, Sy = sum wy, Sxx = sum wx*xc, Sxy = sum wx*yc, Syy = sum wy*yc,
 *   Su = sum w*u, Sxu = sum wx*u, Syu = sum wy*u, Sv = sum w*v, Sxv = sum wx*v, Syv = sum wy*v
 * and solves about the weighted centroid:
 *   !(S0 > 0):  p = 0, model_used = -1, done
 *   mx = Sx/S0, my = Sy/S0, mu = Su/S0, mv = Sv/S0
 *   cxx = Sxx/S0 - mx*mx, cxy = Sxy/S0 - mx*my, cyy = Syy/S0 - my*my
 *   cxu = Sxu/S0 - mx*mu, cyu = Syu/S0 - my*mu, cxv = Sxv/S0 - mx*mv, cyv = Syv/S0 - my*mv
 *   spread = cxx + cyy,  det = cxx*cyy - cxy*cxy
 *   used = model;  AFFINE and !(spread > 1e-9 and det > 1e-9 * (spread*spread)) -> SIMILARITY;
 *                  SIMILARITY and !(spread > 1e-9) -> TRANSLATION
 *   AFFINE:       p1 = (cxu*cyy - cyu*cxy)/det,  p2 = (cyu*cxx - cxu*cxy)/det,
 *                 p4 = (cxv*cyy - cyv*cxy)/det,  p5 = (cyv*cxx - cxv*cxy)/det
 *   SIMILARITY:   a = (cxu + cyv)/spread,  b = (cxv - cyu)/spread;  p1 = a, p2 = -b, p4 = b, p5 = a
 *                 (u = tx + a*xc - b*yc, v = ty + b*xc + a*yc: rotation and isotropic zoom)
 *   TRANSLATION:  p1 = p2 = p4 = p5 = 0
 *   p0 = mu - (p1*mx + p2*my),  p3 = mv - (p4*mx + p5*my)
 * motion[b] (DEVICE memory) gets the record of instance b of a lock-step batch after the last pass: p, weight_sum = S0 of that
 * pass, support = the number of pixels with b > 0, model_used = the model that ran (a model whose rank condition fails falls
 * back to the next simpler one) or -1.
 * Deterministic: the sums run in a fixed order that depends only on (width, height) -- per workgroup of 256 columns x 32 rows
 * a slab of partial sums in the caller's `workspace`, then one workgroup per instance adds the slabs in block order and solves
 * --, so repeated calls, a replayed graph and an instance alone or in its batch give the same bytes.  A pass reads the record
 * of the pass before from `motion` on the device: 2 * (passes) launches on the context's stream, passes = 1 + (sigma > 0 ?
 * iterations : 0), no host round trip, no allocation, no synchronisation, no atomics (graph-capturable).  `workspace` holds at
 * least flow2d_global_motion_workspace_bytes(width, height, instances) bytes, 16-byte aligned.
 * FLOW2D_ERR_INVALID_ARGUMENT for a null flow plane, `motion` or `workspace`, a zero size, a bad pitch, a negative or
 * non-finite sigma, iterations outside [0, 16], an unknown model, a misaligned `motion` (8) or `workspace` (16), a workspace
 * too small, or `motion` / `workspace` bytes -- over every instance of a batch -- that overlap an input plane or each other.
 * Honours flow2d_context_set_batch. */
typedef enum flow2d_motion_model {
    FLOW2D_MOTION_TRANSLATION = 0,
    FLOW2D_MOTION_SIMILARITY = 1,
    FLOW2D_MOTION_AFFINE = 2
} flow2d_motion_model;

typedef struct flow2d_global_motion {
    double p[6];                /* u = (p0 + p1*xc) + p2*yc, v = (p3 + p4*xc) + p5*yc, centred coordinates */
    double weight_sum;          /* S0 of the last pass */
    unsigned long long support; /* pixels with b > 0 */
    int model_used;             /* flow2d_motion_model, or -1: nothing to fit */
    int reserved[3];            /* 0 */
} flow2d_global_motion;

#define FLOW2D_GLOBAL_MOTION_BYTES 80
#define FLOW2D_GLOBAL_MOTION_MAX_ITERATIONS 16
#ifdef __cplusplus
static_assert(sizeof(flow2d_global_motion) == FLOW2D_GLOBAL_MOTION_BYTES, "flow2d_global_motion layout");
#else
_Static_assert(sizeof(flow2d_global_motion) == FLOW2D_GLOBAL_MOTION_BYTES, "flow2d_global_motion layout");
#endif

/* Workspace bytes flow2d_global_motion_2d needs for `instances` lock-step instances of a width x height flow (0 for a zero
 * size).  Host logic only, needs no device. */
FLOW2D_API size_t flow2d_global_motion_workspace_bytes(size_t width, size_t height, size_t instances);
FLOW2D_API int flow2d_global_motion_2d(flow2d_context* ctx, const float* flow_u, const float* flow_v,
                                       const float* mask /* may be NULL */, size_t width, size_t height, size_t pitch_bytes,
                                       int model, double sigma, int iterations, flow2d_global_motion* motion /* device */,
                                       void* workspace, size_t workspace_bytes);

/* The model of a record as planes, and what is left of a flow once it is taken out.  motion: DEVICE memory, record b for
 * instance b.  Every output is optional, at least one is required; for every pixel, with (mu, mv) the model above in double:
 *   model_u = (float)mu, model_v = (float)mv                                 (one rounding)
 *   residual_u = valid ? (float)((double)u - mu) : NaN, residual_v likewise  (valid, u, v as above; NaN = 0x7fc00000; what moves
 *                relative to the global motion)
 *   weight = (float)(sigma > 0 ? b * (s2 / (s2 + (du*du + dv*dv))) : b)      (b, du, dv, s2 as above with the caller's mask and
 *                sigma: the inlier map of a pass that uses this record; a NaN is written as 0x7fc00000)
 * residual_* and weight need both flow planes; model_* alone needs none (flow_u = flow_v = NULL).  Full statistics of the
 * residual: pass model_u / model_v as the "ground truth" of flow2d_flow_error_2d.  One launch, no allocation, no
 * synchronisation (graph-capturable); honours flow2d_context_set_batch.  FLOW2D_ERR_INVALID_ARGUMENT for a null or misaligned
 * `motion`, no output at all, only one plane of a pair (flow, model, residual), residual or weight without the flow, a zero
 * size, a bad pitch, a negative or non-finite sigma, or a written plane whose bytes -- over every instance of a batch --
 * overlap those of an input plane, of the records or of another written plane (the rules of flow2d_compose_flow_2d). */
FLOW2D_API int flow2d_global_flow_2d(flow2d_context* ctx, const flow2d_global_motion* motion /* device */,
                                     const float* flow_u /* may be NULL */, const float* flow_v /* may be NULL */,
                                     const float* mask /* may be NULL */, size_t width, size_t height, size_t pitch_bytes,
                                     double sigma, float* model_u, float* model_v, float* residual_u, float* residual_v,
                                     float* weight);

/* One frame resampled along a global motion (stabilisation): for every pixel x = (x, y)
 *   q = ((float)((double)x + mu), (float)((double)y + mv))          (the model in double, one rounding per component)
 *   ok = 0 <= q.x <= width - 1 and 0 <= q.y <= height - 1           (fp32 comparisons; a NaN or an infinity fails)
 *   output[x] = ok ? S(frame, q) : fill;   valid[x] = ok ? 1 : 0    (when `valid` is not NULL)
 * S: the bilinear sample of flow2d_consistency_2d, the same fp32 operations in the same order; every read stays inside the
 * plane.  With the record of the motion frame a -> frame b and frame = b, output is b brought back onto a's grid.  No flow plane
 * is read: 4 bytes gathered and 4 - 8 written per pixel.  motion: DEVICE memory, record b for instance b.  One launch, no
 * allocation, no synchronisation (graph-capturable); honours flow2d_context_set_batch.  FLOW2D_ERR_INVALID_ARGUMENT for a null
 * or misaligned `motion`, a null `frame` or `output`, a zero size, a bad pitch (the rule of flow2d_consistency_2d), or
 * `output` / `valid` bytes -- over every instance of a batch -- that overlap `frame`, the records or each other.  `fill` may be
 * any float, a NaN included. */
FLOW2D_API int flow2d_warp_global_2d(flow2d_context* ctx, const flow2d_global_motion* motion /* device */, const float* frame,
                                     size_t width, size_t height, size_t pitch_bytes, float fill, float* output,
                                     float* valid /* may be NULL */);

/* Motion segmentation: the independently moving regions of a residual flow, labelled on the device (no reference counterpart;
 * added to ABI version 1 without changing any existing entry).  Connected components of the foreground of a residual flow --
 * what flow2d_global_flow_2d writes as residual_u / residual_v --, numbered, with one record per region.
 *
 * Foreground.  All of this is fp32, each operation rounded on its own (no fused multiply-add).  Per pixel p:
 *   ru = residual_u[p], rv = residual_v[p]
 *   m  = mask ? mask[p] : 0;  if (!(m <= 1)) m = 1;  if (!(m >= 0)) m = 0        (the clamp of flow2d_global_motion_2d: NaN = 1)
 *   fg(p) = (ru*ru + rv*rv > threshold*threshold) && (m < 0.5f)
 * A NaN residual (an invalid vector of flow2d_global_flow_2d) fails the comparison and is background.
 * Edges.  Two 4-neighbours p and q that are both foreground are joined when
 *   (ru_p - ru_q)*(ru_p - ru_q) + (rv_p - rv_q)*(rv_p - rv_q) <= join*join
 * join = +infinity joins every foreground neighbour pair with finite residuals (plain labelling); a finite join keeps two
 * touching objects with different motions apart.  The relation is on edges: a component is a connected component of that
 * graph, so a smooth ramp of residuals is one component even when its two ends differ by far more than `join`.
 * Numbering.  A component's area is its pixel count; components with area < min_area become background (label 0).  The
 * remaining regions are numbered 1, 2, ... in increasing order of their smallest linear index y*width + x.  `labels` is an
 * int plane with the pitch and the batch stride of the float planes; it is always complete, even when there are more regions
 * than max_regions.
 * Records.  regions[k - 1] (DEVICE memory) describes region k for k <= max_regions: area, the sums of the pixel coordinates
 * (centroid = sum / area, done by the caller), the sums over the region's pixels of
 *   llrint((double)clamp(r, -32768.f, 32768.f) * 65536.0)         (round to nearest even; r = ru for sum_u_q16, rv for sum_v_q16)
 * -- the mean residual motion as an exact integer sum, the same bytes in any order of addition; at 2^31 per pixel it cannot
 * overflow below 2^31 pixels --, the inclusive bounding box and the smallest linear index.  Records from
 * min(region_count, max_regions) up to max_regions are zero.  summary[0] (DEVICE memory): region_count (kept regions; may
 * exceed max_regions), foreground (pixels with fg), dropped (foreground pixels in components below min_area), recorded =
 * min(region_count, max_regions), reserved = 0.
 * How: union-find with equivalence by smallest index.  Seven launches on the context's stream whatever the arguments: 64 x 16
 * tiles labelled in LDS, the pairs across tile edges united, the tile roots flattened and the areas summed, the kept roots
 * counted per band of 2048 consecutive indices, one workgroup per instance scanning the bands in order, the records of the
 * roots written, and the labels written with the sums, boxes accumulated per tile in LDS first.  Integer atomics only -- min,
 * max and add on 32- and 64-bit integers: they commute and associate, so the bytes do not depend on the order of arrival; no
 * float atomic anywhere.  No workgroup waits for another.  No host round trip, no allocation, no synchronisation
 * (graph-capturable); repeated calls, a replayed graph and an instance alone or in its batch give the same bytes.  Honours
 * flow2d_context_set_batch: labels and planes at b * stride, regions + b * max_regions, summary + b, one workspace slice per
 * instance.  `workspace` holds at least flow2d_segment_motion_workspace_bytes(width, height, instances) bytes (8 bytes per
 * pixel and 32 per band), 16-byte aligned.
 * FLOW2D_ERR_INVALID_ARGUMENT for a null plane, `labels`, `summary` or `workspace`, regions == NULL with max_regions > 0, a
 * zero size, width*height >= 2^31, a bad pitch (the rule of flow2d_consistency_2d), a negative or NaN threshold, a negative or
 * NaN join (+infinity is allowed), min_area == 0, a misaligned `regions` or `summary` (8) or `workspace` (16), a workspace too
 * small, or a written range -- labels, table, summary, workspace, over every instance of a batch -- that overlaps an input
 * plane or another written range. */
typedef struct flow2d_motion_region {
    unsigned long long area;          /* pixel count */
    unsigned long long sum_x, sum_y;  /* sums of the pixel coordinates */
    long long sum_u_q16, sum_v_q16;   /* sums of the residuals in units of 2^-16 pixel */
    int x0, y0, x1, y1;               /* inclusive bounding box */
    unsigned long long first;         /* smallest linear index y*width + x */
} flow2d_motion_region;

typedef struct flow2d_segment_summary {
    unsigned long long region_count;  /* kept regions; may exceed max_regions */
    unsigned long long foreground;    /* pixels with fg */
    unsigned long long dropped;       /* foreground pixels in components below min_area */
    unsigned recorded;                /* min(region_count, max_regions) */
    unsigned reserved;                /* 0 */
} flow2d_segment_summary;

#define FLOW2D_MOTION_REGION_BYTES 64
#define FLOW2D_SEGMENT_SUMMARY_BYTES 32
#ifdef __cplusplus
static_assert(sizeof(flow2d_motion_region) == FLOW2D_MOTION_REGION_BYTES, "flow2d_motion_region layout");
static_assert(sizeof(flow2d_segment_summary) == FLOW2D_SEGMENT_SUMMARY_BYTES, "flow2d_segment_summary layout");
#else
_Static_assert(sizeof(flow2d_motion_region) == FLOW2D_MOTION_REGION_BYTES, "flow2d_motion_region layout");
_Static_assert(sizeof(flow2d_segment_summary) == FLOW2D_SEGMENT_SUMMARY_BYTES, "flow2d_segment_summary layout");
#endif

/* Workspace bytes flow2d_segment_motion_2d needs for `instances` lock-step instances of a width x height plane (0 for a zero
 * size; a multiple of 16).  Host logic only, needs no device. */
FLOW2D_API size_t flow2d_segment_motion_workspace_bytes(size_t width, size_t height, size_t instances);
FLOW2D_API int flow2d_segment_motion_2d(flow2d_context* ctx, const float* residual_u, const float* residual_v,
                                        const float* mask /* may be NULL */, size_t width, size_t height, size_t pitch_bytes,
                                        float threshold, float join, unsigned min_area, int* labels,
                                        flow2d_motion_region* regions /* device, may be NULL iff max_regions == 0 */,
                                        size_t max_regions, flow2d_segment_summary* summary /* device */, void* workspace,
                                        size_t workspace_bytes);

/* Deformation analysis: how the material a flow describes deforms -- divergence, vorticity, dilatation and the strain tensor
 * with its principal values, from masked differences of the flow (no reference counterpart; added to ABI version 1 without
 * changing any existing entry).  All arithmetic is fp32, every operation rounded on its own (no fused multiply-add), in the
 * order written; sqrtf is correctly rounded.
 *
 * Validity.  For a pixel q inside the frame, with u_q = flow_u[q], v_q = flow_v[q]:
 *   m     = mask ? mask[q] : 0;  if (!(m <= 1)) m = 1;  if (!(m >= 0)) m = 0         (the clamp of flow2d_global_motion_2d: NaN = 1;
 *           `mask` is 1 where the vector is to be left out, as flow2d_consistency_2d writes it)
 *   ok(q) = |u_q| <= 1e9 and |v_q| <= 1e9 and (mask == NULL or m < 0.5f)             (a NaN or an infinity fails)
 * A pixel outside the frame is not ok.
 * Masked differences.  For f in {u, v} at p = (x, y), with L = ok(x-1, y) and R = ok(x+1, y):
 *   L and R:   f_x = (f[x+1] - f[x-1]) * 0.5f
 *   R only:    f_x = f[x+1] - f[x]
 *   L only:    f_x = f[x] - f[x-1]
 *   neither:   no derivative
 * and f_y likewise from (x, y-1) and (x, y+1).  A pixel is valid when ok(p) holds and both axes have a derivative; on an
 * unmasked finite flow this is numpy.gradient(f, edge_order=1) evaluated in fp32.  No difference takes a vector that is not ok
 * into a result: what the caller masked out, and a NaN or an infinity, stay where they are.
 * Quantities.  With a = u_x, b = u_y, c = v_x, d = v_y at a valid pixel:
 *   divergence = a + d
 *   vorticity  = c - b
 *   dilatation = (a + d) + (a*d - b*c)                  (det F - 1 with F = I + grad w: the relative change of area)
 *   measure == FLOW2D_STRAIN_SMALL:           exx = a,  eyy = d,  exy = 0.5f*(b + c)
 *   measure == FLOW2D_STRAIN_GREEN_LAGRANGE:  exx = a + 0.5f*(a*a + c*c),  eyy = d + 0.5f*(b*b + d*d),
 *                                             exy = 0.5f*((b + c) + (a*b + c*d))               (E = (F^T F - I) / 2)
 *   mean = 0.5f*(exx + eyy),  half = 0.5f*(exx - eyy),  max_shear = sqrtf(half*half + exy*exy)
 *   e1 = mean + max_shear,  e2 = mean - max_shear       (the principal strains, e1 >= e2)
 * Outputs.  `out` is a HOST struct of nine device pointers, each of which may be NULL; a requested plane gets its quantity at
 * every valid pixel and NaN (0x7fc00000) at every other pixel of width x height.  Row padding and the container beyond
 * width x height are neither read into a result nor written.  stats[b] (DEVICE memory, may be NULL) gets the record of instance
 * b of a lock-step batch: the counts of valid and invalid pixels and, for each of divergence, vorticity, dilatation, e1, e2 and
 * max_shear over the valid pixels, sum and sum_sq (= the sum of (double)x * (double)x) in double, min and max (updated by
 * x < min and x > max from +inf and -inf; 0 for an empty set); the reserved bytes are 0.  At least one plane or `stats` is
 * required.
 * Deterministic: per workgroup of 64 columns x 16 rows a slab of partial sums in the caller's `workspace`, in a fixed order, then
 * one workgroup per instance adds the slabs in block order; no atomics.  The grid depends only on (width, height), so repeated
 * calls, a replayed graph and an instance alone or in its batch give the same bytes.  Two launches on the context's stream, one
 * when stats == NULL (the workspace is then not used and may be NULL); no allocation, no synchronisation, no host round trip
 * (graph-capturable).  `workspace` holds at least flow2d_deformation_workspace_bytes(width, height, instances) bytes, 16-byte
 * aligned.  Honours flow2d_context_set_batch: planes at b * stride, stats + b.
 * FLOW2D_ERR_INVALID_ARGUMENT for a null flow plane, out == NULL with stats == NULL or an `out` with no plane and no stats,
 * width < 2 or height < 2 (no derivative exists), a bad pitch (the rule of flow2d_consistency_2d), an unknown measure, a
 * misaligned `stats` (8) or `workspace` (16), a null or too small workspace when stats != NULL, or a written range -- a
 * requested plane, the records, the workspace, over every instance of a batch -- that overlaps an input plane or another
 * written range. */
typedef enum flow2d_strain_measure {
    FLOW2D_STRAIN_SMALL = 0,
    FLOW2D_STRAIN_GREEN_LAGRANGE = 1
} flow2d_strain_measure;

typedef struct flow2d_deformation_planes {
    float* divergence;
    float* vorticity;
    float* dilatation;
    float* exx;
    float* eyy;
    float* exy;
    float* e1;
    float* e2;
    float* max_shear;
} flow2d_deformation_planes;

typedef struct flow2d_deformation_moments {
    double sum;
    double sum_sq; /* sum of (double)x * (double)x */
    float min;     /* 0 for an empty set */
    float max;
} flow2d_deformation_moments;

typedef struct flow2d_deformation_stats {
    unsigned long long valid;
    unsigned long long invalid; /* width * height - valid */
    flow2d_deformation_moments divergence, vorticity, dilatation, e1, e2, max_shear;
    unsigned long long reserved[12]; /* 0 */
} flow2d_deformation_stats;

#define FLOW2D_DEFORMATION_STATS_BYTES 256
#ifdef __cplusplus
static_assert(sizeof(flow2d_deformation_stats) == FLOW2D_DEFORMATION_STATS_BYTES, "flow2d_deformation_stats layout");
#else
_Static_assert(sizeof(flow2d_deformation_stats) == FLOW2D_DEFORMATION_STATS_BYTES, "flow2d_deformation_stats layout");
#endif

/* Workspace bytes flow2d_deformation_2d needs for `instances` lock-step instances of a width x height flow when it writes
 * statistics (0 for a zero size; a multiple of 16).  Host logic only, needs no device. */
FLOW2D_API size_t flow2d_deformation_workspace_bytes(size_t width, size_t height, size_t instances);
FLOW2D_API int flow2d_deformation_2d(flow2d_context* ctx, const float* flow_u, const float* flow_v,
                                     const float* mask /* may be NULL */, size_t width, size_t height, size_t pitch_bytes,
                                     int measure, const flow2d_deformation_planes* out /* host, may be NULL */,
                                     flow2d_deformation_stats* stats /* device, may be NULL */, void* workspace,
                                     size_t workspace_bytes);

/* Edge-aware refinement of a flow: a weighted median over a (2 radius + 1)^2 window, guided by an image, that skips unreliable
 * vectors and so gives an occluded pixel the motion of the surface it belongs to (the non-local term of Sun, Roth & Black, CVPR
 * 2010; no reference counterpart; added to ABI version 1 without changing any existing entry).  All arithmetic is fp32, every
 * operation rounded on its own (no fused multiply-add; division correctly rounded), in the order written; no transcendental.
 *
 * Weight of a sample.  For the output pixel x and a window offset (dx, dy), |dx|, |dy| <= radius, the sample is the pixel
 * p = x + (dx, dy).  It takes part when p is inside the frame and |flow_u[p]| <= 1e9 and |flow_v[p]| <= 1e9 (a NaN, an infinity
 * and the unknown-flow value of .flo files fail: the rule of flow2d_flow_error_2d).  Its weight:
 *   m = mask ? mask[p] : 0;  if (!(m <= 1)) m = 1;  if (!(m >= 0)) m = 0            (the clamp of flow2d_global_motion_2d: NaN = 1;
 *                                                                                    `mask` is 1 where the vector is unreliable)
 *   w = 1 - m
 *   guide != NULL and sigma_guide > 0:   d = guide[p] - guide[x];   w = w * sg2 / (sg2 + d*d),   sg2 = sigma_guide * sigma_guide
 *   sigma_space > 0:                     w = w * ss2 / (ss2 + (float)(dx*dx + dy*dy)),            ss2 = sigma_space * sigma_space
 *   q = (int)floorf(4096.f * w), and q = 0 when w is not finite or the sample takes no part
 * The weights are integers of at most 4096: their sum over the window, Q, is exact in 32 bits, and the result depends neither on
 * an order of summation nor on the selection algorithm.
 * Result.  Each component is filtered on its own with the same weights: the output is the smallest sample value x_k among the
 * samples with q > 0 for which 2 * (the summed q of the samples with value <= x_k) >= Q.  A -0 result is written as +0.  Where
 * Q = 0 -- nothing usable in the window -- the input vector is copied bit for bit.  With no guide, no mask and sigma_space = 0 this
 * is the plain median over the part of the window inside the frame (the lower one of an even count).
 * Record.  record[b] (DEVICE memory, may be NULL) gets four counts for instance b of a lock-step batch: pixels (width * height),
 * unfilled (Q = 0), filled (the pixel's own clamped mask value is >= 0.5 and Q > 0; 0 without a mask) and changed (the output
 * differs from the input in the bits of either component).  Integers, added by integer atomics after the entry has zeroed the
 * record on the stream: repeated calls, a replayed graph and an instance alone or in its batch give the same bytes.
 * Row padding and the container beyond width x height are neither read into a result nor written.  One launch on the context's
 * stream (and a 32-byte memset per instance with a record); no allocation, no synchronisation, no host round trip
 * (graph-capturable).  Honours flow2d_context_set_batch: planes at b * stride, record + b.
 * FLOW2D_ERR_INVALID_ARGUMENT for a null flow or output plane, a zero size, a bad pitch (the rule of flow2d_consistency_2d), a
 * radius outside 1 .. FLOW2D_REFINE_MAX_RADIUS, a negative, NaN or infinite sigma, a misaligned `record` (8), or a written range
 * -- out_u, out_v, the records, over every instance of a batch -- that overlaps an input plane or another written range: the
 * filter reads a window, so it cannot run in place. */
#define FLOW2D_REFINE_MAX_RADIUS 7
typedef struct flow2d_refine_record {
    unsigned long long pixels;   /* width * height */
    unsigned long long unfilled; /* Q = 0: the input was copied */
    unsigned long long filled;   /* masked (>= 0.5) pixels that got a value from their window */
    unsigned long long changed;  /* outputs that differ from the input by bits */
} flow2d_refine_record;

#define FLOW2D_REFINE_RECORD_BYTES 32
#ifdef __cplusplus
static_assert(sizeof(flow2d_refine_record) == FLOW2D_REFINE_RECORD_BYTES, "flow2d_refine_record layout");
#else
_Static_assert(sizeof(flow2d_refine_record) == FLOW2D_REFINE_RECORD_BYTES, "flow2d_refine_record layout");
#endif

FLOW2D_API int flow2d_refine_flow_2d(flow2d_context* ctx, const float* flow_u, const float* flow_v,
                                     const float* guide /* may be NULL */, const float* mask /* may be NULL */, size_t width,
                                     size_t height, size_t pitch_bytes, int radius, float sigma_guide, float sigma_space,
                                     float* out_u, float* out_v, flow2d_refine_record* record /* device, may be NULL */);

/* Window correlation (digital image correlation, PIV): the displacement of a (2 radius + 1)^2 window of frame 0 found by an
 * exhaustive search over frame 1 for the largest zero-normalised cross-correlation.  The body of the reference's
 * Methods::Correlation, which it declares and never shipped; added to ABI version 1 without changing any existing entry.
 * The frames are quantised to 8 bits first, so every window sum is an exact integer that depends on no order of summation; only
 * the final score is floating point, a handful of correctly rounded double operations.
 *
 * Quantisation.  For a sample I (fp32), every operation rounded on its own, no fused multiply-add:
 *   t = (I - lo) * scale;   q = 0 when !(t > 0) (a NaN lands here),  q = 255 when t >= 255,  else q = (int)(t + 0.5f)
 * q0 is the quantised frame 0, q1 the quantised frame 1.
 * Nodes.  r = radius (1 .. FLOW2D_CORRELATION_MAX_RADIUS), s = spacing (1 .. FLOW2D_CORRELATION_MAX_SPACING), d = range
 * (1 .. FLOW2D_CORRELATION_MAX_RANGE); N = (2r + 1)^2.  Node (i, j) is centred on pixel (r + i*s, r + j*s);
 * nw = (width - 2r - 1) / s + 1 and nh = (height - 2r - 1) / s + 1 (integer division): flow2d_correlation_grid.  A frame with
 * width < 2r + 1 or height < 2r + 1 holds no node and is an invalid argument.
 * Candidates.  A displacement (dx, dy), |dx| <= d and |dy| <= d, is a candidate of a node when the window centred on
 * (r + i*s + dx, r + j*s + dy) lies inside frame 1 and its V1 > 0.  With S0, S00 the sums of q0 and q0^2 over the node's window,
 * S1, S11 the sums of q1 and q1^2 over the displaced window and S01 the sum of the products q0 * q1 of corresponding pixels, in
 * 64-bit integers
 *   A = N*S01 - S0*S1,   V0 = N*S00 - S0*S0,   V1 = N*S11 - S1*S1,
 *   c = (double)A / sqrt((double)V0 * (double)V1)           (one multiplication, one square root, one division, in double)
 * Peak.  The candidate with the largest c; among equal c the one with the smaller dx*dx + dy*dy, then the smaller dy, then the
 * smaller dx.  Its score is c0.  Per axis, with cm and cp the scores of the neighbours at -1 and +1 along that axis, in double:
 *   den = (cm - 2*c0) + cp;   delta = den < 0 ? (cm - cp) / (2*den) : 0
 * The node is *unrefined* -- delta_x = delta_y = 0 -- when |dx| = d or |dy| = d or any of the four neighbours (dx -+ 1, dy),
 * (dx, dy -+ 1) is not a candidate.  u = (float)((double)dx + delta_x), v = (float)((double)dy + delta_y), score = (float)c0.
 * Invalid and rejected nodes.  V0 = 0 or no candidate at all: u = v = NaN (0x7FC00000), score = 0; the node is *invalid*.
 * Otherwise, score < min_score (compared in fp32; a min_score of -1 rejects nothing): u = v = NaN, the score is kept; the node is
 * *rejected*.
 * Record.  record[b] (DEVICE memory, may be NULL) gets four counts for instance b of a lock-step batch: nodes (nw * nh), invalid,
 * rejected, and unrefined -- the nodes that are neither invalid nor rejected and whose vector is the integer peak for one of the
 * reasons above.  Integers, added by integer atomics after the entry has zeroed the record on the stream: repeated calls, a
 * replayed graph and an instance alone or in its batch give the same bytes.
 * node_u, node_v and node_score (may be NULL) are planes of nw x nh floats with node_pitch_bytes per row (the pitch rule of the
 * frames).  Row padding and the containers beyond width x height and nw x nh are neither read into a result nor written.  One
 * launch on the context's stream (and a 32-byte memset per instance with a record); no allocation, no synchronisation, no host
 * round trip (graph-capturable).  Honours flow2d_context_set_batch: the frames AND the node planes of instance b at b * stride
 * floats from their pointers -- the node planes are laid out like every other plane of the batch, so a stride that holds a frame
 * holds them --, record + b.
 * FLOW2D_ERR_INVALID_ARGUMENT for a null frame, node_u or node_v, a zero size, a bad pitch (the rule of flow2d_consistency_2d,
 * for node_pitch_bytes against nw), a frame smaller than one window, a radius, range or spacing outside its limits, a scale that
 * is not finite and > 0, a lo that is not finite, a NaN min_score, a misaligned record (8), or a written range -- the node planes,
 * the records, over every instance of a batch -- that overlaps a frame or another written range. */
#define FLOW2D_CORRELATION_MAX_RADIUS 15
#define FLOW2D_CORRELATION_MAX_RANGE 32
#define FLOW2D_CORRELATION_MAX_SPACING 64
typedef struct flow2d_correlation_record {
    unsigned long long nodes;     /* nw * nh */
    unsigned long long invalid;   /* V0 = 0 or no candidate: NaN, score 0 */
    unsigned long long rejected;  /* score < min_score: NaN, score kept */
    unsigned long long unrefined; /* delivered vectors without a sub-pixel part */
} flow2d_correlation_record;

#define FLOW2D_CORRELATION_RECORD_BYTES 32
#ifdef __cplusplus
static_assert(sizeof(flow2d_correlation_record) == FLOW2D_CORRELATION_RECORD_BYTES, "flow2d_correlation_record layout");
#else
_Static_assert(sizeof(flow2d_correlation_record) == FLOW2D_CORRELATION_RECORD_BYTES, "flow2d_correlation_record layout");
#endif

/* The node grid of a width x height frame into *nw, *nh (neither may be NULL).  Needs no device.  FLOW2D_ERR_INVALID_ARGUMENT --
 * and nothing written -- for a radius or spacing outside its limits or a frame smaller than one window. */
FLOW2D_API int flow2d_correlation_grid(size_t width, size_t height, int radius, int spacing, size_t* nw, size_t* nh);

FLOW2D_API int flow2d_correlate_2d(flow2d_context* ctx, const float* frame_0, const float* frame_1, size_t width, size_t height,
                                   size_t pitch_bytes, float lo, float scale, int radius, int range, int spacing, float min_score,
                                   float* node_u, float* node_v, float* node_score /* may be NULL */, size_t node_pitch_bytes,
                                   flow2d_correlation_record* record /* device, may be NULL */);

/* A node field of flow2d_correlate_2d brought onto the frame's grid, so that it can feed every consumer of a dense flow
 * (flow2d_flow_error_2d, flow2d_deformation_2d, flow2d_segment_motion_2d, flow2d_refine_flow_2d): bilinear between the four
 * surrounding nodes, over the valid ones only, constant beyond the outermost nodes.  Per pixel (x, y), fp32, every operation
 * rounded on its own (no fused multiply-add; division correctly rounded), with r = radius, s = spacing:
 *   fx = ((float)x - (float)r) / (float)s, clamped to [0, nw - 1];  i0 = (int)floorf(fx);  i1 = min(i0 + 1, nw - 1);
 *   ax = fx - (float)i0;  the same in y with nh (fy, j0, j1, ay)
 *   weights w00 = (1 - ax)*(1 - ay), w10 = ax*(1 - ay), w01 = (1 - ax)*ay, w11 = ax*ay of the nodes (i0, j0), (i1, j0), (i0, j1),
 *   (i1, j1); only nodes whose u and v are both finite take part, in that order:  sw += w;  su += w*u;  sv += w*v  (from 0)
 *   out_u = su / sw, out_v = sv / sw, or NaN (0x7FC00000) for both where !(sw > 0)
 * nw, nh >= 1 are the caller's (any node plane, not only a grid flow2d_correlation_grid would give).  Row padding and the
 * containers beyond nw x nh and width x height are neither read into a result nor written.  One launch on the context's stream;
 * graph-capturable.  Honours flow2d_context_set_batch: node planes and outputs of instance b at b * stride floats.
 * FLOW2D_ERR_INVALID_ARGUMENT for a null plane, a zero size, a bad pitch, a radius outside 0 .. FLOW2D_CORRELATION_MAX_RADIUS, a
 * spacing outside 1 .. FLOW2D_CORRELATION_MAX_SPACING, or an output that overlaps a node plane or the other output, over every
 * instance of a batch. */
FLOW2D_API int flow2d_expand_nodes_2d(flow2d_context* ctx, const float* node_u, const float* node_v, size_t nw, size_t nh,
                                      size_t node_pitch_bytes, int radius, int spacing, float* out_u, float* out_v, size_t width,
                                      size_t height, size_t pitch_bytes);

/* Multi-pass window correlation (multi-grid interrogation with a discrete window offset, Westerweel 1997; the normalised median
 * test, Westerweel & Scarano 2005): the two steps a chain of passes is made of besides flow2d_expand_nodes_2d.  A coarse pass
 * with large windows finds the motion; its validated node field, expanded to the frame's grid, is the *predictor* of the next
 * pass, which searches a small range around it with smaller windows on a denser grid.  Added to ABI version 1 without changing
 * any existing entry.
 *
 * flow2d_correlate_offset_2d: flow2d_correlate_2d with the search of every node centred on an integer offset read from a dense
 * predictor.  Everything not restated here -- quantisation, nodes and grid, the sums, the score, the order of the peak, the
 * parabola, invalid and rejected nodes, the node planes, the pitch rules -- is that entry's text.
 * Predictor.  predictor_u, predictor_v: planes of width x height floats with the frames' pitch, in pixels of the frames; both
 * NULL or both given.  Node (i, j), centred on pixel (cx, cy) = (r + i*s, r + j*s), reads pu = predictor_u[cy][cx] and
 * pv = predictor_v[cy][cx] (a node centre is a pixel: nothing is interpolated).  When pu and pv are both finite, in fp32, every
 * operation rounded on its own:
 *   ox = (int)floorf(fminf(fmaxf(pu, -32768.f), 32768.f) + 0.5f),   oy likewise from pv
 * Otherwise ox = oy = 0 and the node is *unpredicted*.  With NULL predictors every offset is 0 and no node is unpredicted: the
 * node planes and the first four counts are then the bytes of flow2d_correlate_2d.
 * Candidates.  (dx, dy), |dx| <= d and |dy| <= d, is a candidate of the node when the window centred on (cx + ox + dx,
 * cy + oy + dy) lies inside frame 1 and its V1 > 0; S1, S11 and S01 are taken over that window.  The order of the peak compares
 * dx and dy *relative to the offset*, and the node is unrefined when |dx| = d, |dy| = d or one of the four neighbours
 * (dx -+ 1, dy), (dx, dy -+ 1) is no candidate.  Then
 *   u = (float)((double)(ox + dx) + delta_x),   v = (float)((double)(oy + dy) + delta_y),   score = (float)c0
 * (ox + dx in int: exact).  An offset that pushes every candidate out of frame 1 leaves the node invalid.
 * Record.  record[b] (DEVICE memory, may be NULL), 64 bytes: nodes, invalid, rejected, unrefined as in flow2d_correlation_record;
 * unpredicted; candidates -- the number of (node, displacement) pairs that are candidates, over the nodes with V0 > 0 (the work
 * the pass did: each costs N multiply-adds); two reserved words, written as 0.  Integers, added by integer atomics after the
 * entry has zeroed the record on the stream.
 * One launch on the context's stream (and a 64-byte memset per instance with a record); no allocation, no synchronisation, no
 * host round trip (graph-capturable).  Honours flow2d_context_set_batch: frames, predictor planes and node planes of instance b
 * at b * stride floats from their pointers, record + b.
 * FLOW2D_ERR_INVALID_ARGUMENT, and nothing written, for everything flow2d_correlate_2d refuses, one predictor without the other,
 * a predictor that breaks the frames' plane rules, or a written range -- the node planes, the records, over every instance of a
 * batch -- that overlaps a frame, a predictor or another written range; FLOW2D_ERR_UNSUPPORTED for a grid of 2^31 nodes or
 * more. */
typedef struct flow2d_correlation_pass_record {
    unsigned long long nodes;       /* nw * nh */
    unsigned long long invalid;     /* V0 = 0 or no candidate: NaN, score 0 */
    unsigned long long rejected;    /* score < min_score: NaN, score kept */
    unsigned long long unrefined;   /* delivered vectors without a sub-pixel part */
    unsigned long long unpredicted; /* nodes whose predictor was not finite: offset 0 */
    unsigned long long candidates;  /* (node, displacement) pairs scored */
    unsigned long long reserved[2]; /* 0; flow2d_correlate_masked_2d: reserved[0] holds the masked nodes */
} flow2d_correlation_pass_record;

#define FLOW2D_CORRELATION_PASS_RECORD_BYTES 64
#define FLOW2D_CORRELATION_MAX_PASSES 6 /* of the host layer's chain (OpticalFlow2D::CorrelateMultiPass) */
#ifdef __cplusplus
static_assert(sizeof(flow2d_correlation_pass_record) == FLOW2D_CORRELATION_PASS_RECORD_BYTES, "flow2d_correlation_pass_record layout");
#else
_Static_assert(sizeof(flow2d_correlation_pass_record) == FLOW2D_CORRELATION_PASS_RECORD_BYTES, "flow2d_correlation_pass_record layout");
#endif

FLOW2D_API int flow2d_correlate_offset_2d(flow2d_context* ctx, const float* frame_0, const float* frame_1,
                                          const float* predictor_u /* may be NULL */, const float* predictor_v /* with predictor_u */,
                                          size_t width, size_t height, size_t pitch_bytes, float lo, float scale, int radius,
                                          int range, int spacing, float min_score, float* node_u, float* node_v,
                                          float* node_score /* may be NULL */, size_t node_pitch_bytes,
                                          flow2d_correlation_pass_record* record /* device, may be NULL */);

/* The normalised median test of a node field, out of place: every node is judged against the input's neighbours, so the result
 * depends on no order.  Per node (i, j) of the nw x nh field:
 * Neighbours.  The up to eight nodes of the 3 x 3 ring around it that lie inside the grid and whose u and v are both finite; k
 * of them.  A node is *valid* when its own u and v are both finite.
 * Median of k floats (k >= 1): sorted by the floats' order-preserving integer key (b = the float's bits as int32;
 * key = b ^ ((b >> 31) & 0x7FFFFFFF), so -0 < +0) into a[0 .. k-1], the median is (a[(k-1)/2] + a[k/2]) * 0.5f.
 * In fp32, every operation rounded on its own (no fused multiply-add; division correctly rounded):
 *   mu, mv = the medians of the neighbours' u and of their v;   ru = the median of |u_i - mu| over the neighbours, rv alike
 *   for a valid node:  tu = |u - mu| / (ru + epsilon),  tv = |v - mv| / (rv + epsilon);  an *outlier* when tu > threshold || tv > threshold
 * Outcome (out_u, out_v; flag):
 *   k < min_neighbours                                      the node's own bits; 0      -- *unjudged*, valid or not
 *   valid, no outlier                                       the node's own bits; 0
 *   outlier, mode FLOW2D_VALIDATE_FLAG                      NaN (0x7FC00000), NaN; 1
 *   outlier, mode FLOW2D_VALIDATE_REPLACE                   mu, mv; 1
 *   not valid, k >= min_neighbours, FLOW2D_VALIDATE_REPLACE mu, mv; 2           -- *filled*
 *   not valid, k >= min_neighbours, FLOW2D_VALIDATE_FLAG    the node's own bits; 0
 * out_flag (may be NULL) is a float plane that gets 0, 1 or 2.  All planes are nw x nh floats with node_pitch_bytes per row.
 * Record.  record[b] (DEVICE memory, may be NULL), 64 bytes: nodes (nw * nh); judged -- valid nodes with k >= min_neighbours;
 * outliers; filled; unjudged; remaining_invalid -- the nodes whose out_u and out_v are not both finite; two reserved words,
 * written as 0.  Integers, added by integer atomics after the entry has zeroed the record on the stream: alone, in a batch and
 * in a replayed graph the same bytes.
 * Row padding and the containers beyond nw x nh are neither read into a result nor written.  One launch on the context's stream
 * (and a 64-byte memset per instance with a record); no allocation, no synchronisation (graph-capturable).  Honours
 * flow2d_context_set_batch: every plane of instance b at b * stride floats, record + b.
 * FLOW2D_ERR_INVALID_ARGUMENT, and nothing written, for a null node_u, node_v, out_u or out_v, a zero size, a bad pitch, a
 * min_neighbours outside 1 .. 8, a threshold or an epsilon that is not finite and > 0, an unknown mode, a misaligned record (8),
 * or a written range -- outputs, flag, records, over every instance of a batch -- that overlaps an input or another written
 * range; FLOW2D_ERR_UNSUPPORTED for 2^31 nodes or more. */
#define FLOW2D_VALIDATE_FLAG 0
#define FLOW2D_VALIDATE_REPLACE 1
typedef struct flow2d_validation_record {
    unsigned long long nodes;             /* nw * nh */
    unsigned long long judged;            /* valid nodes with k >= min_neighbours */
    unsigned long long outliers;          /* judged nodes that failed the test: flag 1 */
    unsigned long long filled;            /* invalid nodes that took their neighbours' median: flag 2 */
    unsigned long long unjudged;          /* k < min_neighbours: copied */
    unsigned long long remaining_invalid; /* output nodes that are not finite */
    unsigned long long reserved[2];       /* 0; flow2d_validate_nodes_masked_2d: reserved[0] holds the off-specimen nodes */
} flow2d_validation_record;

#define FLOW2D_VALIDATION_RECORD_BYTES 64
#ifdef __cplusplus
static_assert(sizeof(flow2d_validation_record) == FLOW2D_VALIDATION_RECORD_BYTES, "flow2d_validation_record layout");
#else
_Static_assert(sizeof(flow2d_validation_record) == FLOW2D_VALIDATION_RECORD_BYTES, "flow2d_validation_record layout");
#endif

FLOW2D_API int flow2d_validate_nodes_2d(flow2d_context* ctx, const float* node_u, const float* node_v, size_t nw, size_t nh,
                                        size_t node_pitch_bytes, float threshold, float epsilon, int min_neighbours, int mode,
                                        float* out_u, float* out_v, float* out_flag /* may be NULL */,
                                        flow2d_validation_record* record /* device, may be NULL */);

/* The window search and the median test on a region of interest: flow2d_correlate_offset_2d and flow2d_validate_nodes_2d with a
 * pixel mask that says which pixels of frame 0 are not the specimen, so that a region of interest holds through the whole chain
 * and not only in flow2d_subset_refine_masked_2d.  A window that reaches across the specimen's edge is correlated on its specimen
 * pixels alone, and a node off the specimen neither votes in the median test nor is judged by it.  Added to ABI version 1 without
 * changing any existing entry.
 *
 * flow2d_correlate_masked_2d: flow2d_correlate_offset_2d with mask and min_pixels.  Everything not restated here is that entry's
 * text (and through it flow2d_correlate_2d's).
 * mask holds width x height floats with the frames' pitch_bytes, in frame 0's coordinates; in a batch instance b lies at
 * b * stride floats, like the frames.  Frame 1 carries no mask.
 * Excluded.  A pixel is *excluded* when !(m < 0.5), m its mask value compared as a float: 1 means "not the specimen" (the
 * convention of flow2d_subset_refine_masked_2d), and a NaN is excluded.  There is no stencil rule here: the search takes no
 * gradients.
 * Masked.  Nv = the number of pixels of the node's window in frame 0 that are not excluded.  A node is *masked* when its centre
 * pixel (cx, cy) is excluded or !(Nv >= min_pixels).  This test comes before everything else: a masked node reads no predictor
 * (it is never unpredicted), has u = v = NaN (0x7FC00000) and score 0, and counts in `nodes` and in `masked` only.
 * Sums.  S0, S00, S1, S11 and S01 run over the pixels (wx, wy) of the window whose pixel of FRAME 0's window is not excluded --
 * for S1 and S11 the pixels of the candidate's window in frame 1 at the same (wx, wy) -- and Nv stands in the place of N:
 *   A = Nv * S01 - S0 * S1,   V0 = Nv * S00 - S0 * S0,   V1 = Nv * S11 - S1 * S1
 * still exact 64-bit integers (Nv * S01 < 2^36).  Candidates, the score, the order of the peak, the parabola -- whose four
 * neighbours are scored with the same masked sums --, invalid, rejected, unrefined and unpredicted nodes are unchanged.
 * Record.  flow2d_correlation_pass_record, the struct as it is: its seventh word, reserved[0], which the other entries write as
 * 0, holds the count of masked nodes here.  `candidates` counts over the nodes that are neither masked nor have V0 <= 0.
 * Equivalences.  mask == NULL (min_pixels is then not looked at): the call is forwarded to flow2d_correlate_offset_2d.  A mask
 * that excludes nothing: that entry's node planes and all eight record words.
 * One launch on the context's stream (and a 64-byte memset per instance with a record); no allocation, no synchronisation, no
 * host round trip (graph-capturable).  Honours flow2d_context_set_batch: the mask of instance b at b * stride floats, like every
 * other plane.
 * Refusals.  Those of flow2d_correlate_offset_2d, and with a mask also FLOW2D_ERR_INVALID_ARGUMENT, nothing written, for a mask
 * that breaks the frames' plane rules, a written range -- over every instance of a batch -- that overlaps the mask, or a
 * min_pixels outside 1 .. (2r + 1)^2. */
FLOW2D_API int flow2d_correlate_masked_2d(flow2d_context* ctx, const float* frame_0, const float* frame_1,
                                          const float* predictor_u /* may be NULL */, const float* predictor_v /* with predictor_u */,
                                          size_t width, size_t height, size_t pitch_bytes, float lo, float scale, int radius,
                                          int range, int spacing, float min_score, const float* mask /* device, may be NULL */,
                                          int min_pixels, float* node_u, float* node_v, float* node_score /* may be NULL */,
                                          size_t node_pitch_bytes, flow2d_correlation_pass_record* record /* device, may be NULL */);

/* flow2d_validate_nodes_masked_2d: flow2d_validate_nodes_2d with the pixel mask and the geometry of the grid the nodes lie on:
 * mask is a plane of width x height floats with pitch_bytes per row (in a batch instance b at b * stride floats), and node (i, j)
 * is centred on pixel (cx, cy) = (radius + i * spacing, radius + j * spacing).  nw x nh must be what flow2d_correlation_grid
 * answers for (width, height, radius, spacing).
 * Off the specimen.  A node is *off the specimen* when mask[cy][cx] is excluded (!(m < 0.5)).  Such a node is never a neighbour,
 * whatever its vector holds.  It comes out as NaN (0x7FC00000), NaN with flag 3 (FLOW2D_VALIDATE_FLAG_MASKED) in either mode, and
 * counts in `nodes` and in the record's seventh word, reserved[0] ("masked": the other entries write it as 0; the struct stays
 * as it is), and in no other word: `remaining_invalid` counts on-specimen outputs only.
 * Every other node gets the text of flow2d_validate_nodes_2d over the neighbours that remain.
 * Equivalences.  mask == NULL (the geometry is then not looked at): the call is forwarded to flow2d_validate_nodes_2d.  A mask
 * that excludes no node centre: that entry's bytes, the record included.
 * One launch; graph-capturable; honours flow2d_context_set_batch.
 * Refusals.  Those of flow2d_validate_nodes_2d, and with a mask also FLOW2D_ERR_INVALID_ARGUMENT, nothing written, for a mask that
 * breaks the plane rules with (width, height, pitch_bytes), a radius or spacing outside its limits, a frame smaller than one
 * window, an nw x nh that is not the grid of that geometry, or a written range -- over every instance of a batch -- that overlaps
 * the mask. */
#define FLOW2D_VALIDATE_FLAG_MASKED 3
FLOW2D_API int flow2d_validate_nodes_masked_2d(flow2d_context* ctx, const float* node_u, const float* node_v, size_t nw, size_t nh,
                                               size_t node_pitch_bytes, float threshold, float epsilon, int min_neighbours, int mode,
                                               const float* mask /* device, may be NULL */, size_t width, size_t height,
                                               size_t pitch_bytes, int radius, int spacing, float* out_u, float* out_v,
                                               float* out_flag /* may be NULL */,
                                               flow2d_validation_record* record /* device, may be NULL */);

/* Subset refinement of a node field (digital image correlation): the inverse-compositional Gauss-Newton iteration with a
 * first-order shape function (Baker & Matthews 2004; Pan, Li & Tong 2013) on the zero-mean normalised sum of squared differences.
 * Every node of a field that flow2d_correlate_2d, flow2d_correlate_offset_2d or flow2d_validate_nodes_2d delivered is refined from
 * its vector (u0, v0) to a displacement with its four gradients, p = (u, ux, uy, v, vx, vy): the point (cx + xi, cy + eta) of
 * frame 0 lies at (cx + xi + u + ux*xi + uy*eta, cy + eta + v + vx*xi + vy*eta) in frame 1.  Added to ABI version 1 without
 * changing any existing entry.
 *
 * The frames are used as they are, fp32, not quantised.  Everything below is IEEE double (a sample or an argument is converted
 * first, which is exact); every operation is rounded on its own, no fused multiply-add; division and square root correctly
 * rounded.  Every test is written as a positive comparison, so that a NaN fails it.
 * Nodes.  r = grid_radius (1 .. FLOW2D_CORRELATION_MAX_RADIUS) and s = spacing (1 .. FLOW2D_CORRELATION_MAX_SPACING) say where
 * the nodes are: node (i, j) of the nw x nh planes is centred on pixel (cx, cy) = (r + i*s, r + j*s), and the grid must lie inside
 * the frame as flow2d_correlation_grid would lay it: (nw - 1)*s + 2r + 1 <= width, (nh - 1)*s + 2r + 1 <= height.
 * R = subset_radius (1 .. FLOW2D_SUBSET_MAX_RADIUS) is the subset's, N = (2R + 1)^2.  Pixel k = 0 .. N - 1 of the subset has
 * xi = k mod (2R + 1) - R and eta = k div (2R + 1) - R.  K = max_iterations (1 .. FLOW2D_SUBSET_MAX_ITERATIONS).
 * A *sum over the subset* is a sum of N terms; the order in which they are added is the one thing this text leaves open.
 * State of a node (out_state, a float plane): n >= 1 converged in iteration n; 0 not converged after K iterations; -1 *no input*;
 * -2 *flat*; -3 *strayed*.  The first that applies, in the order of this text, ends the node.
 * No input.  u0 or v0 is not finite.
 * Frame-0 window.  *Strayed* unless cx - R >= 0, cy - R >= 0, cx + R <= width - 1 and cy + R <= height - 1 (possible when R > r).
 * Frame-0 quantities, per pixel k at (x, y) = (cx + xi, cy + eta):
 *   f = frame_0[y][x];   fx = (frame_0[y][min(x + 1, width - 1)] - frame_0[y][max(x - 1, 0)]) * 0.5;   fy likewise with rows
 *   fm = (sum of f) / N;   fd = f - fm;   Df2 = sum of fd*fd;   *flat* when !(Df2 > 0);   Df = sqrt(Df2)
 * Hessian.  J = (J0 .. J5) = (fx, fx*xi, fx*eta, fy, fy*xi, fy*eta), each a rounded product;  H[a][b] = sum of J[a]*J[b].
 * Cholesky H = L L^T, column k = 0 .. 5 in turn; every inner sum starts from 0 and adds its terms from m = 0 up:
 *   d = H[k][k] - (sum over m < k of L[k][m]*L[k][m]);   *flat* when !(d > 1e-10 * H[k][k]);   L[k][k] = sqrt(d)
 *   for i = k + 1 .. 5:   L[i][k] = (H[i][k] - (sum over m < k of L[i][m]*L[k][m])) / L[k][k]
 * Solve(b), the x with H x = b; inner sums from 0, terms from the lowest m up:
 *   for i = 0 .. 5:        y[i] = (b[i] - (sum over m < i of L[i][m]*y[m])) / L[i][i]
 *   for i = 5 down to 0:   x[i] = (y[i] - (sum over m = i + 1 .. 5 of L[m][i]*x[m])) / L[i][i]
 * Start.  p = (u0, 0, 0, v0, 0, 0).
 * Iteration n = 1 .. K (it *begins* here):
 *   1. Positions.  X = (double)(cx + xi) + ((u + ux*xi) + uy*eta);   Y = (double)(cy + eta) + ((v + vx*xi) + vy*eta).
 *      *Strayed* unless every pixel of the subset has X >= 0, X <= width - 1, Y >= 0 and Y <= height - 1.
 *   2. Sampling.  g = the Catmull-Rom sample of frame 1 at (X, Y).  ix = floor(X), t = X - ix; the taps are columns ix - 1 ..
 *      ix + 2, each clamped to [0, width - 1], with the weights
 *        w0 = ((-0.5*t + 1)*t - 0.5)*t;   w1 = ((1.5*t - 2.5)*t)*t + 1;   w2 = ((-1.5*t + 2)*t + 0.5)*t;   w3 = ((0.5*t - 0.5)*t)*t
 *      A row a0 .. a3 gives ((w0*a0 + w1*a1) + w2*a2) + w3*a3.  Rows iy - 1 .. iy + 2 (iy = floor(Y), clamped to [0, height - 1])
 *      are combined in the same way with the weights of Y - iy.
 *   3. Residual.  gm = (sum of g) / N;   gd = g - gm;   Dg2 = sum of gd*gd;   *flat* when !(Dg2 > 0);   Dg = sqrt(Dg2);
 *      c = (sum of fd*gd) / (Df*Dg);   q = Df / Dg;   res = fd - q*gd;   b[a] = sum of J[a]*res;   x = Solve(b);
 *      (du, dux, duy, dv, dvx, dvy) = (-x[0], .. , -x[5]).
 *   4. Update, p <- W(p) o W(dp)^-1.   a = 1 + dux, b = duy, c' = dvx, d = 1 + dvy;   det = a*d - b*c';
 *      *strayed* when !(|det| > 1e-12);   ia = d/det, ib = (-b)/det, ic = (-c')/det, id = a/det;
 *      tx = -(ia*du + ib*dv);   ty = -(ic*du + id*dv);   p11 = 1 + ux, p12 = uy, p21 = vx, p22 = 1 + vy;
 *      u <- (p11*tx + p12*ty) + u;   v <- (p21*tx + p22*ty) + v;
 *      ux <- (p11*ia + p12*ic) - 1;   uy <- p11*ib + p12*id;   vx <- p21*ia + p22*ic;   vy <- (p21*ib + p22*id) - 1
 *      (all six from the old p).
 *   5. Stop.  *Strayed* unless |u - u0| <= max_shift, |v - v0| <= max_shift and |ux|, |uy|, |vx|, |vy| <= max_gradient
 *      (the new p).  Converged, state n, when
 *        sqrt(((((du*du + (R*dux)*(R*dux)) + (R*duy)*(R*duy)) + dv*dv) + (R*dvx)*(R*dvx)) + (R*dvy)*(R*dvy)) < epsilon
 *      (epsilon = 0: never, all K iterations run and the state is 0).
 * Outputs.  State >= 0: u, v, the gradients and the last c (out_score), each cast to float.  No input: u, v and the gradients NaN
 * (0x7FC00000), score 0.  Flat and strayed: u0 and v0 copied bit for bit, the gradients 0, score 0.  The four gradient planes
 * are given all or none; out_score and out_state may be NULL.  All node planes are nw x nh floats with node_pitch_bytes per row.
 * Record.  record[b] (DEVICE memory, may be NULL), 64 bytes: nodes (nw * nh); converged; unconverged (state 0); strayed; flat;
 * no_input; iterations -- iterations begun, over all nodes --; one reserved word, written as 0.  Integers, added by integer
 * atomics after the entry has zeroed the record on the stream: alone, in a batch and in a replayed graph the same bytes.
 * Row padding and the containers beyond width x height and nw x nh are neither read into a result nor written.  One launch on the
 * context's stream (and a 64-byte memset per instance with a record); no allocation, no synchronisation (graph-capturable).
 * Honours flow2d_context_set_batch: frames and node planes of instance b at b * stride floats from their pointers, record + b.
 * FLOW2D_ERR_INVALID_ARGUMENT, and nothing written, for a null frame, node_u0, node_v0, out_u or out_v, a zero size, a bad pitch
 * (the rule of flow2d_consistency_2d, for node_pitch_bytes against nw), a grid_radius, spacing, subset_radius or max_iterations
 * outside its limits, a grid that does not lie inside the frame, an epsilon that is not finite and >= 0, a max_shift or
 * max_gradient that is not finite and > 0, gradient planes given in part, a misaligned record (8), or a written range -- the
 * outputs, the records, over every instance of a batch -- that overlaps a frame, an input node plane or another written range;
 * FLOW2D_ERR_UNSUPPORTED for 2^31 nodes or more. */
#define FLOW2D_SUBSET_MAX_RADIUS 15
#define FLOW2D_SUBSET_MAX_ITERATIONS 64
typedef struct flow2d_subset_record {
    unsigned long long nodes;       /* nw * nh */
    unsigned long long converged;   /* state >= 1 */
    unsigned long long unconverged; /* state 0: K iterations without convergence, p delivered */
    unsigned long long strayed;     /* state -3 */
    unsigned long long flat;        /* state -2 */
    unsigned long long no_input;    /* state -1 */
    unsigned long long iterations;  /* iterations begun, over all nodes */
    unsigned long long reserved;    /* 0; flow2d_subset_refine_masked_2d: the masked nodes, state -4 */
} flow2d_subset_record;

#define FLOW2D_SUBSET_RECORD_BYTES 64
#ifdef __cplusplus
static_assert(sizeof(flow2d_subset_record) == FLOW2D_SUBSET_RECORD_BYTES, "flow2d_subset_record layout");
#else
_Static_assert(sizeof(flow2d_subset_record) == FLOW2D_SUBSET_RECORD_BYTES, "flow2d_subset_record layout");
#endif

FLOW2D_API int flow2d_subset_refine_2d(flow2d_context* ctx, const float* frame_0, const float* frame_1, size_t width, size_t height,
                                       size_t pitch_bytes, const float* node_u0, const float* node_v0, size_t nw, size_t nh,
                                       size_t node_pitch_bytes, int grid_radius, int spacing, int subset_radius, int max_iterations,
                                       float epsilon, float max_shift, float max_gradient, float* out_u, float* out_v,
                                       float* out_ux /* the four gradient planes: all or none */, float* out_uy, float* out_vx,
                                       float* out_vy, float* out_score /* may be NULL */, float* out_state /* may be NULL */,
                                       flow2d_subset_record* record /* device, may be NULL */);

/* Subset refinement started from a whole deformation: flow2d_subset_refine_2d with four more input planes, node_ux0, node_uy0,
 * node_vx0 and node_vy0 -- the start's gradients, given all or none, nw x nh floats with node_pitch_bytes per row like node_u0.
 * It is what a loading sequence needs: every frame is correlated against the same reference frame, and the previous step's
 * result (through flow2d_predict_nodes_2d) is the next step's start, so that a subset that has rotated or stretched too far
 * for a rigid window search is still found.  Added to ABI version 1 without changing any existing entry.
 * The text of flow2d_subset_refine_2d holds word for word except at four places:
 * No input.  u0, v0, ux0, uy0, vx0 or vy0 is not finite.
 * Start.  p = (u0, ux0, uy0, v0, vx0, vy0), each converted to double.
 *   (5. Stop is unchanged: the displacement is bounded against (u0, v0), the gradients absolutely by max_gradient, so a start
 *   with a gradient beyond max_gradient strays in iteration 1 unless that iteration brings it back.)
 * Outputs.  Flat and strayed: u0, v0 and the four start gradients copied bit for bit, score 0 -- the field stays usable as the
 * next step's input.
 * Refusals.  Also FLOW2D_ERR_INVALID_ARGUMENT, and nothing written, for start planes given in part, a start plane that breaks
 * the node planes' rules, or a written range that overlaps a start plane.
 * With all four start planes NULL every output byte and the record are those of flow2d_subset_refine_2d. */
FLOW2D_API int flow2d_subset_refine_from_2d(flow2d_context* ctx, const float* frame_0, const float* frame_1, size_t width,
                                            size_t height, size_t pitch_bytes, const float* node_u0, const float* node_v0,
                                            const float* node_ux0 /* the four start gradients: all or none */,
                                            const float* node_uy0, const float* node_vx0, const float* node_vy0, size_t nw, size_t nh,
                                            size_t node_pitch_bytes, int grid_radius, int spacing, int subset_radius,
                                            int max_iterations, float epsilon, float max_shift, float max_gradient, float* out_u,
                                            float* out_v, float* out_ux /* the four gradient planes: all or none */, float* out_uy,
                                            float* out_vx, float* out_vy, float* out_score /* may be NULL */,
                                            float* out_state /* may be NULL */, flow2d_subset_record* record /* device, may be NULL */);

/* Masked subset refinement, digital image correlation on a region of interest: flow2d_subset_refine_from_2d with one more input
 * plane, mask, which says which pixels of frame 0 are not the specimen -- the background beside a dog-bone, the inside of a hole
 * --, and min_pixels.  A subset that reaches across the specimen's edge is refined on its specimen pixels alone.  Added to ABI
 * version 1 without changing any existing entry.
 * mask holds width x height floats with the frames' pitch_bytes, in frame 0's coordinates; in a batch instance b lies at
 * b * stride floats, like the frames.
 * Everything not named here is the text of flow2d_subset_refine_from_2d word for word: the arithmetic in IEEE double with every
 * operation rounded on its own, the positive comparisons, the Catmull-Rom sample, Cholesky and Solve, the update, the stop test
 * with R, the outputs of the states >= 0, -1, -2 and -3, batches and graph capture.
 * Excluded.  A pixel is *excluded* when !(m < 0.5), m its mask value compared as a float: 1 means "do not use" (the convention of
 * the occlusion masks), and a NaN is excluded.
 * Usable.  Pixel (x, y) is *usable* when none of (x, y), (min(x + 1, width - 1), y), (max(x - 1, 0), y), (x, min(y + 1, height - 1))
 * and (x, max(y - 1, 0)) is excluded: the pixel itself and the four its fx and fy read.
 * States.  One more, -4 *masked* (FLOW2D_SUBSET_STATE_MASKED).  The tests run in this order:
 *   1. *Masked* when the centre pixel (cx, cy) is excluded -- before *no input*: an off-specimen node is masked whatever its start holds.
 *   2. *No input*, as flow2d_subset_refine_from_2d has it.
 *   3. The frame-0 window test (*strayed*), as there.
 *   4. Nv = the number of usable pixels of the subset.  *Masked* when !(Nv >= min_pixels).
 * Sums.  The usable pixels form a list m = 0 .. Nv - 1 in ascending k.  Every *sum over the subset* is a sum over that list, of
 * Nv terms, and Nv stands where N stood (fm, gm).  Positions are formed, tested against the frame (1. Positions) and sampled only
 * for the usable pixels.  The order in which a sum's terms are added stays the one thing this text leaves open.
 * Outputs.  Masked: u, v and the four gradients NaN (0x7FC00000), score 0, state -4; the node adds no iterations.
 * Record.  The eighth word of record[b], which the other entries write as 0 (flow2d_subset_record::reserved: the struct stays as it
 * is), holds the count of masked nodes here.
 * Equivalences.  mask == NULL (min_pixels is then not looked at): every output byte and the record are those of
 * flow2d_subset_refine_from_2d -- the call is forwarded.  A mask that excludes nothing: every output byte and the record are again
 * those of flow2d_subset_refine_from_2d; the list is then k itself.
 * Refusals.  Those of flow2d_subset_refine_from_2d, and with a mask also FLOW2D_ERR_INVALID_ARGUMENT, nothing written, for a
 * min_pixels outside FLOW2D_SUBSET_MIN_PIXELS .. (2R + 1)^2 (six unknowns need six pixels), a mask that breaks the frames' plane
 * rules, or a written range that overlaps the mask. */
#define FLOW2D_SUBSET_STATE_MASKED (-4)
#define FLOW2D_SUBSET_MIN_PIXELS 6
FLOW2D_API int flow2d_subset_refine_masked_2d(flow2d_context* ctx, const float* frame_0, const float* frame_1, size_t width,
                                              size_t height, size_t pitch_bytes, const float* node_u0, const float* node_v0,
                                              const float* node_ux0 /* the four start gradients: all or none */,
                                              const float* node_uy0, const float* node_vx0, const float* node_vy0, size_t nw, size_t nh,
                                              size_t node_pitch_bytes, int grid_radius, int spacing, int subset_radius,
                                              int max_iterations, float epsilon, float max_shift, float max_gradient,
                                              const float* mask /* device, may be NULL */, int min_pixels, float* out_u, float* out_v,
                                              float* out_ux /* the four gradient planes: all or none */, float* out_uy, float* out_vx,
                                              float* out_vy, float* out_score /* may be NULL */, float* out_state /* may be NULL */,
                                              flow2d_subset_record* record /* device, may be NULL */);

/* Subset refinement with a second-order shape function (Lu & Cary 2000; Gao, Cheng, Su, Xu, Zhang & Zhang 2015): the
 * inverse-compositional Gauss-Newton iteration of flow2d_subset_refine_2d with twelve parameters,
 *   p = (u, ux, uy, uxx, uxy, uyy, v, vx, vy, vxx, vxy, vyy) = (p0 .. p11):
 * the point (cx + xi, cy + eta) of frame 0 lies at
 *   X = cx + xi + u + ux*xi + uy*eta + uxx*xi^2/2 + uxy*xi*eta + uyy*eta^2/2,   Y likewise with v,
 * in frame 1 -- a subset that bends, where the first-order refinement is biased by the mean of the quadratic term over the
 * subset.  Added to ABI version 1 without changing any existing entry.
 * Everything not named here is the text of flow2d_subset_refine_2d word for word: the node and grid rules, the frame-0
 * quantities, the residual and the Catmull-Rom sampling, the five states and their order, positive comparisons everywhere, IEEE
 * double with every operation rounded on its own, the order of a sum over the subset as the one thing left open, the record,
 * batches, graph capture and the refusals.  What differs:
 * R = subset_radius runs from 2 to FLOW2D_SUBSET_MAX_RADIUS: nine pixels cannot carry twelve unknowns.
 * Shape.  phi = (phi0 .. phi5) = (1, xi, eta, 0.5*xi*xi, xi*eta, 0.5*eta*eta) -- every one exact, as is every product
 *   phi[a]*phi[b] (at most 15^4 / 4).
 * No input.  u0, v0 or a start value that is given is not finite.
 * Hessian, 12 x 12.  J[a] = fx*phi[a] and J[6 + a] = fy*phi[a] (a = 0 .. 5), each a rounded product, are what b is formed from;
 *   H is formed from the products of the gradients first:  wxx = fx*fx, wxy = fx*fy, wyy = fy*fy, each rounded, and
 *   H[a][b] = sum of wxx*(phi[a]*phi[b]);   H[a][6 + b] = H[6 + b][a] = sum of wxy*(phi[a]*phi[b]);
 *   H[6 + a][6 + b] = sum of wyy*(phi[a]*phi[b])        (a, b = 0 .. 5).
 *   phi[a]*phi[b] = phi[b]*phi[a] bit for bit, so each of the three 6 x 6 blocks is symmetric in (a, b) as stated, not only up
 *   to rounding: 3 x 21 different sums, not 78.
 * Cholesky and Solve: the text's with 12 in the place of 6 (k = 0 .. 11, i up to 11), the same pivot test, *flat*.
 * Start.  p = (u0, ux0, uy0, uxx0, uxy0, uyy0, v0, vx0, vy0, vxx0, vxy0, vyy0), each converted to double; the four start
 *   gradients are given all or none, the six start curvatures all or none and only with the gradients; an absent value is 0.
 * Iteration n = 1 .. K:
 *   1. Positions.  X = (double)(cx + xi) + (((((u + ux*phi1) + uy*phi2) + uxx*phi3) + uxy*phi4) + uyy*phi5);   Y likewise with
 *      (double)(cy + eta) and v, vx, ...  *Strayed* as in the text.
 *   2. Sampling: the text's.
 *   3. Residual: the text's, with b[a] = sum of J[a]*res for a = 0 .. 11, x = Solve(b), dp[a] = -x[a].
 *   4. Update, p <- W(p) o W(dp)^-1.  A warp acts on the monomials (xi^2, xi*eta, eta^2, xi, eta, 1) as a 6 x 6 matrix.  For a
 *      parameter vector q let A(q) = (a1 .. a6) = (0.5*uxx, uxy, 0.5*uyy, 1 + ux, uy, u) and B(q) = (b1 .. b6) =
 *      (0.5*vxx, vxy, 0.5*vyy, vx, 1 + vy, v).  The rows W0 .. W5 of W(dp), from A = A(dp) and B = B(dp), each product of two
 *      rows truncated at second order in (xi, eta):
 *        W0 = (a4*a4 + 2*(a1*a6),  2*(a4*a5) + 2*(a2*a6),  a5*a5 + 2*(a3*a6),  2*(a4*a6),  2*(a5*a6),  a6*a6)
 *        W1 = ((a4*b4 + a1*b6) + a6*b1,  ((a4*b5 + a5*b4) + a2*b6) + a6*b2,  (a5*b5 + a3*b6) + a6*b3,  a4*b6 + a6*b4,
 *              a5*b6 + a6*b5,  a6*b6)
 *        W2 = W0 with b in the place of a;   W3 = A;   W4 = B;   W5 = (0, 0, 0, 0, 0, 1).
 *      Only the rows A and B of W(p) W(dp)^-1 are needed: the z with z W(dp) = A(p), and the z' with z' W(dp) = B(p) (the old
 *      p).  W5 leaves z5 out of the first five columns, so z0 .. z4 solve the 5 x 5 system M z = rhs with M[j][i] = W_i[j] and
 *      rhs[j] = A(p)[j] (i, j = 0 .. 4), by elimination without pivoting -- W(dp) is a perturbation of the identity --, both
 *      right-hand sides at once:
 *        for k = 0 .. 4:   *strayed* when !(|M[k][k]| > 1e-6);   for j = k + 1 .. 4:   f = M[j][k] / M[k][k];
 *          M[j][i] = M[j][i] - f*M[k][i] for i = k + 1 .. 4;   rhs[j] = rhs[j] - f*rhs[k]
 *        for i = 4 down to 0:   z[i] = (rhs[i] - (sum over m = i + 1 .. 4 of M[i][m]*z[m])) / M[i][i]
 *          (the sum from 0, terms from the lowest m up)
 *        z[5] = A(p)[5] - ((((z[0]*W0[5] + z[1]*W1[5]) + z[2]*W2[5]) + z[3]*W3[5]) + z[4]*W4[5])
 *      All five pivots are tested -- the k = 4 one too, which has no row below it -- before anything is divided by them.
 *      The new p:  uxx = 2*z[0], uxy = z[1], uyy = 2*z[2], ux = z[3] - 1, uy = z[4], u = z[5];
 *      vxx = 2*z'[0], vxy = z'[1], vyy = 2*z'[2], vx = z'[3], vy = z'[4] - 1, v = z'[5].
 *   5. Stop.  *Strayed* unless |u - u0| <= max_shift, |v - v0| <= max_shift, |ux|, |uy|, |vx|, |vy| <= max_gradient and
 *      |uxx|, |uxy|, |uyy|, |vxx|, |vxy|, |vyy| <= max_curvature (the new p).  With R2 = (double)(R*R), hR2 = 0.5*R2 and
 *      t = (dp0, R*dp1, R*dp2, hR2*dp3, R2*dp4, hR2*dp5, dp6, R*dp7, R*dp8, hR2*dp9, R2*dp10, hR2*dp11), converged, state n, when
 *        sqrt(((..((t0*t0 + t1*t1) + t2*t2) + ..) + t11*t11) < epsilon       (the squares added in the order 0 .. 11).
 * Outputs.  out_u, out_v; the four gradient planes out_ux, out_uy, out_vx, out_vy, all or none; the six curvature planes
 * out_uxx, out_uxy, out_uyy, out_vxx, out_vxy, out_vyy, all or none (with or without the gradient planes); out_score and
 * out_state, each optional.  State >= 0: p and the last c, each cast to float.  No input: the twelve NaN (0x7FC00000), score 0.
 * Flat and strayed: the whole start copied bit for bit -- a start value that was absent comes back as 0 --, score 0.
 * The four plane groups -- start_gradients, start_curvatures, out_gradients, out_curvatures -- are HOST arrays of four or six
 * device pointers, read during the call and not kept; a NULL array and an array of NULLs both mean that the group is absent.
 * Refusals.  Those of flow2d_subset_refine_from_2d, with subset_radius < 2 among them, and also: a max_curvature that is not
 * finite and > 0, curvature planes or start curvatures given in part, start curvatures without start gradients, a start or
 * output plane that breaks the node planes' rules, and a written range that overlaps any start plane or another written one. */
#define FLOW2D_SUBSET2_MIN_RADIUS 2
FLOW2D_API int flow2d_subset_refine2_2d(flow2d_context* ctx, const float* frame_0, const float* frame_1, size_t width, size_t height,
                                        size_t pitch_bytes, const float* node_u0, const float* node_v0,
                                        const float* const* start_gradients /* NULL, or ux0, uy0, vx0, vy0: all or none */,
                                        const float* const* start_curvatures /* NULL, or uxx0, uxy0, uyy0, vxx0, vxy0, vyy0 */,
                                        size_t nw, size_t nh, size_t node_pitch_bytes, int grid_radius, int spacing,
                                        int subset_radius, int max_iterations, float epsilon, float max_shift, float max_gradient,
                                        float max_curvature, float* out_u, float* out_v,
                                        float* const* out_gradients /* NULL, or ux, uy, vx, vy: all or none */,
                                        float* const* out_curvatures /* NULL, or uxx, uxy, uyy, vxx, vxy, vyy: all or none */,
                                        float* out_score /* may be NULL */, float* out_state /* may be NULL */,
                                        flow2d_subset_record* record /* device, may be NULL */);

/* Cubic B-spline interpolation of the deformed frame (Unser, Aldroubi & Eden 1993; Schreier, Braasch & Sutton 2000 on the
 * interpolation bias of DIC): the coefficients of a plane, and the two subset refinements sampling them in the place of the
 * Catmull-Rom sample of frame 1.  Added to ABI version 1 without changing any existing entry.
 * The arithmetic follows the rule of flow2d_subset_refine_2d's text: IEEE double, every operation rounded on its own, no fused
 * multiply-add, positive comparisons.
 *
 * flow2d_bspline_prefilter_2d: dst = the cubic B-spline coefficients of src, times 36 -- see *Scale*.  The recursive filter is
 * replaced by its symmetric impulse response truncated at H = FLOW2D_BSPLINE_HORIZON = 16 (|Z|^16 is about 7e-10, far below an
 * fp32 ulp): every output depends on 33 x 33 inputs only, and nothing depends on a scan order.
 * reflect(i, n): 0 when n = 1; otherwise p = 2(n - 1), m = i mod p taken non-negative, and the result is m when m <= n - 1, else
 *   p - m.  Whole-sample mirroring, as often as it takes (n may be below 16).
 * Constants, in double:  Z = sqrt(3.0) - 2.0;   z[0] = 1, z[j] = z[j - 1] * Z for j = 1 .. 16;   G = sqrt(3.0) / 6.0.
 * A line s[0 .. n - 1] gives d[k], k = 0 .. n - 1:
 *   acc = 0;   for j = 16 down to 1:  acc = acc + z[j] * (s[reflect(k - j, n)] + s[reflect(k + j, n)]);
 *   acc = acc + s[k];   d[k] = G * acc.
 * Rows first, on the floats converted to double; then columns on the rows' doubles, which are not rounded to float in between;
 * the result is cast to float.
 * Scale.  With G per axis a constant plane c gives c / 36: the sampler's weights below are six times the B-spline's per axis, so
 *   that no division occurs per sample.
 * One launch on the context's stream, no allocation, no synchronisation (graph-capturable); no atomics: alone, in a batch and in
 * a replayed graph the same bytes.  Honours flow2d_context_set_batch (src and dst of instance b at b * stride floats).  Row
 * padding and the containers beyond width x height are neither read into a result nor written.
 * FLOW2D_ERR_INVALID_ARGUMENT, and nothing written, for a null pointer, a zero size, a bad pitch (the rule of
 * flow2d_consistency_2d) or a dst that overlaps src, over every instance of a batch. */
#define FLOW2D_BSPLINE_HORIZON 16
FLOW2D_API int flow2d_bspline_prefilter_2d(flow2d_context* ctx, const float* src, float* dst, size_t width, size_t height,
                                           size_t pitch_bytes);

/* flow2d_subset_refine_masked_2d on the coefficients of frame 1: coeff_1, where frame_1 stands there, is a plane that
 * flow2d_bspline_prefilter_2d made from frame 1 (same width, height and pitch_bytes; in a batch instance b at b * stride floats).
 * The text of flow2d_subset_refine_masked_2d (and through it that of flow2d_subset_refine_from_2d) holds word for word except
 *   2. Sampling.  g = the cubic B-spline sample of coeff_1 at (X, Y).  ix = floor(X), t = X - ix, u = 1.0 - t;
 *        W0 = (u*u)*u;   W1 = ((3.0*t - 6.0)*t)*t + 4.0;   W2 = ((3.0*u - 6.0)*u)*u + 4.0;   W3 = (t*t)*t
 *      The taps are columns reflect(ix - 1 + i, width), i = 0 .. 3, of coeff_1 -- reflected, not clamped: the extension the
 *      prefilter assumed.  A row a0 .. a3 gives ((W0*a0 + W1*a1) + W2*a2) + W3*a3.  Rows reflect(iy - 1 + j, height) (iy =
 *      floor(Y)) are combined in the same way with the weights of Y - iy.
 * Frame 0's quantities, the central differences fx and fy among them, do not change.  The start gradients are given all or none.
 * mask == NULL (min_pixels is then not looked at): the bytes of a mask that excludes nothing.
 * Refusals.  Those of flow2d_subset_refine_masked_2d with coeff_1 in the place of frame_1: a coeff_1 that is null or breaks the
 * frames' plane rules, or that meets a written range. */
FLOW2D_API int flow2d_subset_refine_spline_2d(flow2d_context* ctx, const float* frame_0, const float* coeff_1, size_t width,
                                              size_t height, size_t pitch_bytes, const float* node_u0, const float* node_v0,
                                              const float* node_ux0 /* the four start gradients: all or none */,
                                              const float* node_uy0, const float* node_vx0, const float* node_vy0, size_t nw, size_t nh,
                                              size_t node_pitch_bytes, int grid_radius, int spacing, int subset_radius,
                                              int max_iterations, float epsilon, float max_shift, float max_gradient,
                                              const float* mask /* device, may be NULL */, int min_pixels, float* out_u, float* out_v,
                                              float* out_ux /* the four gradient planes: all or none */, float* out_uy, float* out_vx,
                                              float* out_vy, float* out_score /* may be NULL */, float* out_state /* may be NULL */,
                                              flow2d_subset_record* record /* device, may be NULL */);

/* flow2d_subset_refine2_2d on the coefficients of frame 1: its text word for word with coeff_1 in the place of frame_1 and
 * 2. Sampling replaced by that of flow2d_subset_refine_spline_2d.  It takes no mask. */
FLOW2D_API int flow2d_subset_refine2_spline_2d(flow2d_context* ctx, const float* frame_0, const float* coeff_1, size_t width,
                                               size_t height, size_t pitch_bytes, const float* node_u0, const float* node_v0,
                                               const float* const* start_gradients /* NULL, or ux0, uy0, vx0, vy0: all or none */,
                                               const float* const* start_curvatures /* NULL, or uxx0, uxy0, uyy0, vxx0, vxy0, vyy0 */,
                                               size_t nw, size_t nh, size_t node_pitch_bytes, int grid_radius, int spacing,
                                               int subset_radius, int max_iterations, float epsilon, float max_shift,
                                               float max_gradient, float max_curvature, float* out_u, float* out_v,
                                               float* const* out_gradients /* NULL, or ux, uy, vx, vy: all or none */,
                                               float* const* out_curvatures /* NULL, or uxx, uxy, uyy, vxx, vxy, vyy: all or none */,
                                               float* out_score /* may be NULL */, float* out_state /* may be NULL */,
                                               flow2d_subset_record* record /* device, may be NULL */);

/* The uncertainty of a first-order refinement's nodes: per node the covariance of p = (u, ux, uy, v, vx, vy) as the Gauss-Newton
 * least squares gives it, Cov(p) ~ s2 * H^-1 (Sutton, Orteu & Schreier 2009, ch. 5; Wang, Sutton et al. 2009) -- the residual
 * variance s2 of the ZNSSD at the node's p times the inverse of the Hessian the refinement factors.  One evaluation per node, no
 * iteration.  It estimates the RANDOM error the frames' noise puts into p; it says nothing about the interpolation bias of the
 * sample (a noise-free pair gives the interpolation residual's small s2, not 0 bias).  Added to ABI version 1 without changing
 * any existing entry.
 * Inputs.  frame_0; frame_1, which is frame 1 with interpolation = 0 (the Catmull-Rom sample, the sampling rules of
 * flow2d_subset_refine_masked_2d word for word) and frame 1's coefficients, as flow2d_bspline_prefilter_2d made them, with
 * interpolation = 1 (the cubic B-spline sample, the rules of flow2d_subset_refine_spline_2d word for word).  The six node planes
 * node_u, node_v, node_ux, node_uy, node_vx, node_vy of a first-order refinement and its state plane node_state, all required,
 * nw x nh floats with node_pitch_bytes per row.  grid_radius, spacing and subset_radius (1 .. FLOW2D_SUBSET_MAX_RADIUS) as in
 * flow2d_subset_refine_2d; min_state (0 or 1).  mask (may be NULL) and min_pixels as in flow2d_subset_refine_masked_2d: *excluded*
 * and *usable* are that text's, and without a mask every pixel of the subset is usable and min_pixels is not looked at.
 * Everything below is IEEE double with every operation rounded on its own, no fused multiply-add, division and square root
 * correctly rounded, every test a positive comparison, as in flow2d_subset_refine_2d's text; the order in which the terms of a
 * *sum over the subset* are added is again the one thing left open.
 * Per node, the first rule that applies ends it:
 *   1. *Masked*: the centre pixel (cx, cy) is excluded (only with a mask).
 *   2. *Skipped*: !(state >= (float)min_state), or any of the six inputs is not finite.  The states
 *      FLOW2D_SUBSET_STATE_PREDICTED (65) and FLOW2D_SUBSET_STATE_COMPOSED (66) pass, so that a predicted or composed field can
 *      be evaluated against the frames it refers to.
 *   3. *Outside*: the frame-0 window test of flow2d_subset_refine_2d fails.
 *   4. With a mask: Nv = the number of usable pixels; *masked* when !(Nv >= min_pixels).  N stands for Nv below and every sum
 *      runs over the list of usable pixels in ascending k.
 *   5. *Thin*: !(N >= 9).  The degrees of freedom are N - 8: the six shape parameters, and the offset and the scale of the ZNSSD.
 *   6. The frame-0 quantities, J, H, Cholesky and Solve exactly as flow2d_subset_refine_2d's text has them.  *Flat* when
 *      !(Df2 > 0) or when a pivot fails its test.
 *   7. p = the six inputs, each converted to double.  Positions X, Y as in step 1 of that text's iteration.  *Outside* unless
 *      every one of them has X >= 0, X <= width - 1, Y >= 0 and Y <= height - 1.
 *   8. g sampled at (X, Y).  gm = (sum of g) / N;   gd = g - gm;   Dg2 = sum of gd*gd;   *flat* when !(Dg2 > 0);
 *      Dg = sqrt(Dg2);   q = Df / Dg;   res = fd - q*gd.
 *   9. S = sum of res*res;   s2 = S / (double)(N - 8).
 *  10. x_a = Solve(e_a) for a = 0 .. 5, e_a the a-th unit vector: the columns of H^-1.
 *  11. sigma_u = sqrt(s2 * x_0[0]);   sigma_v = sqrt(s2 * x_3[3]);   sigma_ux, sigma_uy, sigma_vx, sigma_vy likewise from
 *      x_1[1], x_2[2], x_4[4], x_5[5].
 *  12. rho = x_0[3] / sqrt(x_0[0] * x_3[3]), the correlation of u and v.
 *  13. noise = sqrt(s2), in grey values: what the residual says the noise of fd - q*gd is.  Each output is cast to float.
 * Outputs, nw x nh floats with node_pitch_bytes per row: out_sigma_u, out_sigma_v (required); out_rho (may be NULL); the four
 * gradient sigmas, all or none; out_noise (may be NULL).  A node that ends early gets NaN (0x7FC00000) in every plane given.
 * Record.  record[b] (DEVICE memory, may be NULL), 64 bytes: nodes (nw * nh); evaluated; skipped; masked; outside; flat; thin;
 * one reserved word, written as 0.  Integers, added by integer atomics after the entry has zeroed the record on the stream:
 * alone, in a batch and in a replayed graph the same bytes.
 * Row padding and the containers beyond width x height and nw x nh are neither read into a result nor written.  One launch on the
 * context's stream (and a 64-byte memset per instance with a record); no allocation, no synchronisation (graph-capturable).
 * Honours flow2d_context_set_batch: frames, mask and node planes of instance b at b * stride floats, record + b.
 * FLOW2D_ERR_INVALID_ARGUMENT, and nothing written, for a null frame, input plane, out_sigma_u or out_sigma_v, a zero size, a bad
 * pitch (the rule of flow2d_consistency_2d), an interpolation or min_state that is neither 0 nor 1, a grid_radius, spacing or
 * subset_radius outside its limits, a grid that does not lie inside the frame, with a mask a min_pixels outside
 * FLOW2D_SUBSET_MIN_PIXELS .. (2R + 1)^2 or a mask that breaks the frames' plane rules, gradient sigmas given in part, a
 * misaligned record (8), or a written range -- the outputs, the records, over every instance of a batch -- that overlaps a
 * frame, the mask, an input plane or another written range; FLOW2D_ERR_UNSUPPORTED for 2^31 nodes or more. */
typedef struct flow2d_uncertainty_record {
    unsigned long long nodes;     /* nw * nh */
    unsigned long long evaluated; /* nodes with a covariance */
    unsigned long long skipped;   /* state below min_state, or an input that is not finite */
    unsigned long long masked;    /* centre excluded, or fewer than min_pixels usable pixels */
    unsigned long long outside;   /* the subset leaves frame 0, or a position leaves frame 1 */
    unsigned long long flat;      /* Df2 or Dg2 not positive, or a pivot failed */
    unsigned long long thin;      /* fewer than nine usable pixels */
    unsigned long long reserved;  /* 0 */
} flow2d_uncertainty_record;

#define FLOW2D_UNCERTAINTY_RECORD_BYTES 64
#ifdef __cplusplus
static_assert(sizeof(flow2d_uncertainty_record) == FLOW2D_UNCERTAINTY_RECORD_BYTES, "flow2d_uncertainty_record layout");
#else
_Static_assert(sizeof(flow2d_uncertainty_record) == FLOW2D_UNCERTAINTY_RECORD_BYTES, "flow2d_uncertainty_record layout");
#endif

FLOW2D_API int flow2d_subset_uncertainty_2d(flow2d_context* ctx, const float* frame_0,
                                            const float* frame_1 /* interpolation 1: its B-spline coefficients */,
                                            int interpolation /* 0 Catmull-Rom, 1 B-spline */, size_t width, size_t height,
                                            size_t pitch_bytes, const float* node_u, const float* node_v, const float* node_ux,
                                            const float* node_uy, const float* node_vx, const float* node_vy,
                                            const float* node_state, size_t nw, size_t nh, size_t node_pitch_bytes, int grid_radius,
                                            int spacing, int subset_radius, int min_state,
                                            const float* mask /* device, may be NULL */, int min_pixels, float* out_sigma_u,
                                            float* out_sigma_v, float* out_rho /* may be NULL */,
                                            float* out_sigma_ux /* the four gradient sigmas: all or none */, float* out_sigma_uy,
                                            float* out_sigma_vx, float* out_sigma_vy, float* out_noise /* may be NULL */,
                                            flow2d_uncertainty_record* record /* device, may be NULL */);

/* The start of the next step of a sequence from a step's result, out of place: a node the refinement found is kept, every other
 * node is predicted from its neighbours.  Every node is judged against the input, so the result depends on no order.
 * Inputs: the six planes node_u, node_v, node_ux, node_uy, node_vx, node_vy and node_state (the outputs of
 * flow2d_subset_refine_2d / flow2d_subset_refine_from_2d, or of an earlier call of this entry), nw x nh floats with
 * node_pitch_bytes per row; s = spacing (1 .. FLOW2D_CORRELATION_MAX_SPACING), the pixels between neighbouring nodes;
 * min_state (0 or 1); min_neighbours (1 .. 8).
 * Usable.  A node is *usable* when state >= (float)min_state (a positive comparison: a NaN state fails) and its u, v, ux, uy, vx
 * and vy are all finite.  min_state = 1 takes only converged (and predicted) nodes, 0 also those that ran out of iterations.
 * Kept.  A usable node: the six values and the state copied bit for bit.
 * Predicted.  Any other node (i, j) looks at its eight neighbours (i + di, j + dj) in the fixed order (di, dj) = (-1,-1), (0,-1),
 * (1,-1), (-1,0), (1,0), (-1,1), (0,1), (1,1); those that lie inside the grid and are usable *in the input* count, m of them.
 * Everything below is IEEE double (an input is converted first, which is exact), every operation rounded on its own, no fused
 * multiply-add.  Neighbour n offers six candidates: with dx = (double)(-di*s) and dy = (double)(-dj*s) (the products in int)
 *   cu = (u_n + ux_n*dx) + uy_n*dy;   cv = (v_n + vx_n*dx) + vy_n*dy;   ux_n, uy_n, vx_n, vy_n as they are.
 * With m >= min_neighbours each of the six outputs is the median of its m candidates, cast to float: the candidates are put in
 * order by < -- c comes before c' when c < c', and candidates of which neither is below the other (equal ones, -0 and +0)
 * keep the neighbours' order -- into c[0 .. m-1]; the median is c[m div 2] for odd m and (c[m div 2 - 1] + c[m div 2]) * 0.5 for
 * even m.  out_state = FLOW2D_SUBSET_STATE_PREDICTED (65, one above FLOW2D_SUBSET_MAX_ITERATIONS), so that a second pass
 * treats the node as usable at either min_state.
 * Empty.  With m < min_neighbours all six outputs are NaN (0x7FC00000) and out_state = -1 (no input).
 * out_state may be NULL.  Record.  record[b] (DEVICE memory, may be NULL), 64 bytes: nodes (nw * nh); kept; predicted; empty;
 * four reserved words, written as 0.  Integers, added by integer atomics after the entry has zeroed the record on the stream:
 * alone, in a batch and in a replayed graph the same bytes.
 * Row padding and the containers beyond nw x nh are neither read into a result nor written.  One launch on the context's stream
 * (and a 64-byte memset per instance with a record); no allocation, no synchronisation (graph-capturable).  Honours
 * flow2d_context_set_batch: every plane of instance b at b * stride floats, record + b.
 * FLOW2D_ERR_INVALID_ARGUMENT, and nothing written, for a null input plane or a null one of the six output planes, a zero size,
 * a bad pitch, a spacing, min_state or min_neighbours outside its limits, a misaligned record (8), or a written range -- outputs,
 * state, records, over every instance of a batch -- that overlaps an input or another written range; FLOW2D_ERR_UNSUPPORTED for
 * 2^31 nodes or more. */
#define FLOW2D_SUBSET_STATE_PREDICTED 65
typedef struct flow2d_predict_record {
    unsigned long long nodes;       /* nw * nh */
    unsigned long long kept;        /* usable nodes, copied */
    unsigned long long predicted;   /* nodes that took their neighbours' medians: state 65 */
    unsigned long long empty;       /* fewer than min_neighbours usable neighbours: NaN, state -1 */
    unsigned long long reserved[4]; /* 0 */
} flow2d_predict_record;

#define FLOW2D_PREDICT_RECORD_BYTES 64
#ifdef __cplusplus
static_assert(sizeof(flow2d_predict_record) == FLOW2D_PREDICT_RECORD_BYTES, "flow2d_predict_record layout");
#else
_Static_assert(sizeof(flow2d_predict_record) == FLOW2D_PREDICT_RECORD_BYTES, "flow2d_predict_record layout");
#endif

FLOW2D_API int flow2d_predict_nodes_2d(flow2d_context* ctx, const float* node_u, const float* node_v, const float* node_ux,
                                       const float* node_uy, const float* node_vx, const float* node_vy, const float* node_state,
                                       size_t nw, size_t nh, size_t node_pitch_bytes, int spacing, int min_state, int min_neighbours,
                                       float* out_u, float* out_v, float* out_ux, float* out_uy, float* out_vx, float* out_vy,
                                       float* out_state /* may be NULL */, flow2d_predict_record* record /* device, may be NULL */);

/* Strain on the node grid (digital image correlation): the nine quantities of flow2d_deformation_2d from a node field's
 * displacement gradients, which are either the gradients a subset refinement delivered (window = 0) or the gradient of a
 * low-order polynomial fitted by least squares to the displacements of the usable nodes inside a *strain window* around each
 * node (Pan, Asundi, Xie & Gao, Opt. Eng. 48 (2009): pointwise least squares).  Nodes that were lost are left out of the fit,
 * so holes and the border of the grid are handled by the fit itself.  Added to ABI version 1 without changing any existing entry.
 *
 * Everything below is IEEE double (an input is converted first, which is exact); every operation is rounded on its own, no
 * fused multiply-add; division and square root correctly rounded.  Every test is written as a positive comparison, so that a
 * NaN fails it.
 * Inputs.  node_u, node_v; node_state (may be NULL); node_ux, node_uy, node_vx, node_vy (all or none): nw x nh floats with
 * node_pitch_bytes per row.  s = spacing (1 .. FLOW2D_CORRELATION_MAX_SPACING), the pixels between neighbouring nodes;
 * m = window (0 .. FLOW2D_NODE_STRAIN_MAX_WINDOW), the strain window's radius in nodes; order (1 or 2); min_nodes; min_state
 * (0 or 1); measure (a flow2d_strain_measure).
 * Usable.  A node q is *usable* when it lies inside the grid, node_state == NULL or state[q] >= (float)min_state, u_q and v_q
 * are finite and, when m = 0, its four gradients are finite.  A node that is not usable is *invalid*, with the reason *centre*.
 * m = 0 (direct).  a, b, c, d = ux, uy, vx, vy of the node.  The gradient planes are required; order and min_nodes are not
 * looked at.
 * m >= 1 (window fit).  The gradient planes are not read and may be NULL.  The basis phi over a window offset (di, dj),
 * |di|, |dj| <= m, is (1, di, dj) for order 1, k = 3, and (1, di, dj, di*di, di*dj, dj*dj) for order 2, k = 6; the products are
 * formed in int.  min_nodes lies in k .. (2m + 1)^2.  The usable nodes q = (i + di, j + dj) of the window of node (i, j) are
 * visited in raster order, dj ascending and within that di ascending; n is their count (the centre is one of them).
 *   M[a][b] = sum of phi_a*phi_b, in 64-bit integers, then converted (exact);
 *   wu = (double)u_q - (double)u_centre,  wv likewise;
 *   bu[a] = sum of phi_a*wu, each product rounded, the terms added from 0 in the visiting order;  bv[a] likewise.
 * *Sparse*, invalid, when !(n >= min_nodes).  Otherwise the Cholesky factorisation and Solve of flow2d_subset_refine_2d's text
 * with M in the place of H and k in the place of 6 (columns 0 .. k - 1, i up to k - 1); the node is *degenerate*, invalid, where
 * that text says *flat*: when !(d > 1e-10 * M[kk][kk]) in some column kk.  Collinear nodes end here.  Otherwise
 *   cu = Solve(bu),  cv = Solve(bv);   a = cu[1]/s,  b = cu[2]/s,  c = cv[1]/s,  d = cv[2]/s,   s converted to double.
 * Quantities, in double, each cast to float once at the end:
 *   divergence = a + d;   vorticity = c - b;   dilatation = (a + d) + (a*d - b*c)
 *   measure == FLOW2D_STRAIN_SMALL:           exx = a,  eyy = d,  exy = 0.5*(b + c)
 *   measure == FLOW2D_STRAIN_GREEN_LAGRANGE:  exx = a + 0.5*(a*a + c*c),  eyy = d + 0.5*(b*b + d*d),
 *                                             exy = 0.5*((b + c) + (a*b + c*d))
 *   mean = 0.5*(exx + eyy),  half = 0.5*(exx - eyy),  max_shear = sqrt(half*half + exy*exy),  e1 = mean + max_shear,
 *   e2 = mean - max_shear      (exx, eyy and exy enter these as doubles, before their cast)
 * Outputs.  `out` is a HOST struct of nine device pointers to planes ON THE NODE GRID (nw x nh, node_pitch_bytes), each of which
 * may be NULL; a requested plane gets its quantity at every valid node and NaN (0x7FC00000) at every other node of nw x nh.
 * Row padding and the containers beyond nw x nh are neither read into a result nor written.  stats[b] (DEVICE memory, may be
 * NULL) gets the record of instance b with the layout and meaning of flow2d_deformation_stats over the valid nodes -- valid,
 * invalid (nw * nh - valid) and sum, sum_sq, min, max of the six floats that are (or would be) stored -- and three of the
 * reserved words: reserved[0] = *centre* nodes, reserved[1] = *sparse* nodes, reserved[2] = *degenerate* nodes; the rest 0.
 * Deterministic: per workgroup of 64 x 4 nodes a slab of partial sums in the caller's `workspace`, then one workgroup per
 * instance adds the slabs in block order; no atomics.  The grid depends only on (nw, nh): repeated calls, a replayed graph and
 * an instance alone or in its batch give the same bytes.  Two launches on the context's stream, one when stats == NULL (the
 * workspace is then not used and may be NULL); no allocation, no synchronisation (graph-capturable).  `workspace` holds at
 * least flow2d_node_strain_workspace_bytes(nw, nh, instances) bytes, 16-byte aligned.  Honours flow2d_context_set_batch: planes
 * at b * stride, stats + b.
 * FLOW2D_ERR_INVALID_ARGUMENT, and nothing written, for a null node_u or node_v, out == NULL or without a plane when stats ==
 * NULL, a zero size, a bad pitch (the rule of flow2d_consistency_2d, for node_pitch_bytes against nw), a spacing, window,
 * min_state or measure outside its limits, for m >= 1 an order or min_nodes outside its limits, m = 0 without the gradient
 * planes, gradient planes given in part, a misaligned `stats` (8) or `workspace` (16), a null or too small workspace when stats
 * != NULL, or a written range -- a requested plane, the records, the workspace, over every instance of a batch -- that overlaps
 * an input plane or another written range; FLOW2D_ERR_UNSUPPORTED for 2^31 nodes or more. */
#define FLOW2D_NODE_STRAIN_MAX_WINDOW 7
/* Workspace bytes flow2d_node_strain_2d needs for `instances` lock-step instances of an nw x nh grid when it writes statistics
 * (0 for a zero size; a multiple of 16).  Host logic only, needs no device. */
FLOW2D_API size_t flow2d_node_strain_workspace_bytes(size_t nw, size_t nh, size_t instances);
FLOW2D_API int flow2d_node_strain_2d(flow2d_context* ctx, const float* node_u, const float* node_v,
                                     const float* node_state /* may be NULL */,
                                     const float* node_ux /* the four gradient planes: all or none */, const float* node_uy,
                                     const float* node_vx, const float* node_vy, size_t nw, size_t nh, size_t node_pitch_bytes,
                                     int spacing, int window, int order, int min_nodes, int min_state, int measure,
                                     const flow2d_deformation_planes* out /* host, may be NULL */,
                                     flow2d_deformation_stats* stats /* device, may be NULL */, void* workspace,
                                     size_t workspace_bytes);

/* Robust strain windows: the window fit of flow2d_node_strain_2d as iteratively reweighted least squares with a Cauchy weight
 * (Holland & Welsch, Commun. Stat. A6 (1977)), so that a node which was delivered as usable but lies in a wrong place neither
 * bends the windows that hold it nor goes unnoticed.  Added to ABI version 1 without changing any existing entry.
 *
 * Everything flow2d_node_strain_2d defines for m >= 1 holds -- IEEE double, every operation rounded on its own, every test a
 * positive comparison; the inputs (without the gradient planes, which a window fit does not read), usable nodes, the basis, the
 * visiting order, wu and wv against the centre, n, *sparse* when !(n >= min_nodes) before anything is factored, the
 * factorisation, the solves, the quantities, the planes, the record and its reduction -- with these additions.
 * Inputs in addition.  sigma, a float, finite and > 0, in pixels; s2 = sigma*sigma after converting sigma to double.
 * K = iterations (0 .. FLOW2D_NODE_STRAIN_MAX_ITERATIONS), the reweighted passes.  window = 0 is refused: the direct form has
 * nothing to reweight.
 * Passes t = 0 .. K.  Every tap q (a usable node of the window) carries a weight w_q in double; in pass 0, w_q = 1.
 *   M[a][b] = sum of w_q * (double)(phi_a*phi_b), the product of the basis formed in int;
 *   bu[a] = sum of (w_q * (double)phi_a) * wu,  bv[a] likewise;   every term rounded as written, added from 0 in visiting order.
 * Factor M and solve cu = Solve(bu), cv = Solve(bv) as in flow2d_node_strain_2d; a failed pivot test in any pass makes the node
 * *degenerate*.  The residuals of the pass, per tap:
 *   ru = wu - (sum over a ascending, from 0, of cu[a]*(double)phi_a),  rv likewise,  r2 = ru*ru + rv*rv;
 * for t < K the next pass has w_q = s2 / (s2 + r2).  (With every w_q = 1.0 the sums are flow2d_node_strain_2d's: integers below
 * 2^53 and products by 1.0.  K = 0 with a sigma no residual reaches gives that entry's planes and record.)
 * After pass K.  A tap is *kept* when r2 <= s2, with the residuals of pass K; kept is their count.  A node with
 * !(kept >= min_nodes) is *sparse* (the existing reason and counter).  Otherwise a, b, c, d come from cu, cv of pass K as in
 * flow2d_node_strain_2d.  A node that reached this point -- valid, or sparse by its kept count -- is *finished*.  A finished node
 * whose own centre tap is not kept is *suspect*; a valid one still gets its strain, which is its neighbours' fit.
 * Outputs in addition.  `diagnostics` (a HOST struct of three device pointers, may be NULL, each may be NULL): planes on the node
 * grid like those of `out`, NaN (0x7FC00000) at an invalid node and at a valid one
 *   residual = (float)sqrt((sum of r2 over the kept taps, from 0 in visiting order) / (double)kept),
 *   rejected = (float)(n - kept),     centre = (float)sqrt(r2 of the centre tap).
 * stats[b]: the record of flow2d_node_strain_2d and, counted over the finished nodes, reserved[3] = nodes with n - kept > 0,
 * reserved[4] = the sum of their rejected taps n - kept, reserved[5] = suspect nodes; the rest 0.  (Not over the valid nodes
 * alone: a window whose passes lock onto its outlier keeps too few taps and is sparse, and that is the node these words are
 * there to report; the planes hold NaN there like at every invalid node.)  The same two ordered launches with
 * slabs of flow2d_node_strain_robust_workspace_bytes: the same bytes alone, in a lock-step batch and under graph replay.
 * FLOW2D_ERR_INVALID_ARGUMENT, and nothing written, for what flow2d_node_strain_2d refuses (a diagnostic plane counts as a
 * requested plane: alone it is output enough, and it may overlap neither an input nor another written range), for window = 0,
 * a sigma that is not finite or <= 0, or iterations outside their limits; FLOW2D_ERR_UNSUPPORTED for 2^31 nodes or more. */
#define FLOW2D_NODE_STRAIN_MAX_ITERATIONS 16
typedef struct flow2d_node_strain_diagnostics {
    float* residual; /* RMS residual of the kept taps, pixels */
    float* rejected; /* usable taps of the window that were not kept */
    float* centre;   /* the node's own residual, pixels */
} flow2d_node_strain_diagnostics;
/* Workspace bytes flow2d_node_strain_robust_2d needs for `instances` lock-step instances of an nw x nh grid when it writes
 * statistics (0 for a zero size; a multiple of 16).  Host logic only, needs no device. */
FLOW2D_API size_t flow2d_node_strain_robust_workspace_bytes(size_t nw, size_t nh, size_t instances);
FLOW2D_API int flow2d_node_strain_robust_2d(flow2d_context* ctx, const float* node_u, const float* node_v,
                                            const float* node_state /* may be NULL */, size_t nw, size_t nh, size_t node_pitch_bytes,
                                            int spacing, int window, int order, int min_nodes, int min_state, int measure, float sigma,
                                            int iterations, const flow2d_deformation_planes* out /* host, may be NULL */,
                                            const flow2d_node_strain_diagnostics* diagnostics /* host, may be NULL */,
                                            flow2d_deformation_stats* stats /* device, may be NULL */, void* workspace,
                                            size_t workspace_bytes);

/* Weighted strain windows: the window fit of flow2d_node_strain_2d as a Gauss-Markov fit whose weights are the inverse variances
 * flow2d_subset_uncertainty_2d delivers per node (Aitken, Proc. R. Soc. Edinburgh 55 (1935)), the standard deviations of the
 * strain from the inverse of the matrices the fit factors, and optionally the reweighted passes of flow2d_node_strain_robust_2d
 * with a scale in sigmas instead of pixels.  Added to ABI version 1 without changing any existing entry.
 *
 * Everything flow2d_node_strain_2d defines for m >= 1 holds -- IEEE double, every operation rounded on its own, no fused
 * multiply-add, every test a positive comparison, taps visited in raster order; the inputs (without the gradient planes), usable
 * nodes, the basis, wu and wv against the centre, the Cholesky factorisation, Solve, the quantities, the planes, the record and
 * its reduction -- with these additions.
 * Inputs in addition.  node_sigma_u, node_sigma_v (required): planes on the node grid, the out_sigma_u and out_sigma_v of
 * flow2d_subset_uncertainty_2d, in pixels.  sigma_floor, a float, finite and >= 0, in pixels: a variance every node has beside
 * the one reported (the uncertainty estimates the random error only: an exact match reports +0, and the sampler's bias is not
 * in it); f2 = sigma_floor*sigma_floor after converting it to double.  T = threshold, a float, finite and >= 0, in sigmas;
 * t2 = T*T after converting T to double; T = 0: no robust part.  K = iterations (0 .. FLOW2D_NODE_STRAIN_MAX_ITERATIONS), which
 * must be 0 when T = 0.  window = 0 is refused.
 * Weighable.  For a usable node q, with sigma_u and sigma_v converted to double,
 *   vu_q = sigma_u*sigma_u + f2,   vv_q = sigma_v*sigma_v + f2.
 * q is *weighable* when vu_q > 0, vv_q > 0, vu_q < +inf and vv_q < +inf (a NaN sigma fails; a sigma of 0 needs a floor; only
 * the square of a sigma is looked at), and then pu_q = 1.0 / vu_q,  pv_q = 1.0 / vv_q.  Only weighable nodes of the window are
 * taps and are visited; n is their count.  A node that is not weighable is invalid with the reason *centre*, like one that is
 * not usable.  *Sparse* when !(n >= min_nodes), before anything is factored.
 * Passes t = 0 .. K.  Every tap carries c_q in double; in pass 0, c_q = 1.  u and v are separate least-squares fits:
 *   Mu[a][b] = sum of (c_q*pu_q) * (double)(phi_a*phi_b), the product of the basis formed in int;
 *   bu[a] = sum of ((c_q*pu_q) * (double)phi_a) * wu;
 *   Mv and bv likewise with pv_q and wv;   every term rounded as written, added from 0 in visiting order.
 * Factor Mu and solve cu = Solve_Mu(bu); factor Mv and solve cv = Solve_Mv(bv); a failed pivot test in either matrix in any pass
 * makes the node *degenerate*.  The residuals of the pass, per tap, ru and rv as in flow2d_node_strain_robust_2d, and
 *   r2 = (ru*ru)*pu_q + (rv*rv)*pv_q      (dimensionless: the squared distance from the fit in the tap's own sigmas);
 * for t < K the next pass has c_q = t2 / (t2 + r2).
 * After pass K.  With T > 0 a tap is *kept* when r2 <= t2, with the residuals of pass K; with T = 0 every tap is kept.  *Sparse*
 * by !(kept >= min_nodes), *finished* and *suspect* (a finished node whose own tap is not kept: never with T = 0) are those of
 * flow2d_node_strain_robust_2d; a, b, c, d come from cu and cv of pass K as in flow2d_node_strain_2d.
 * Covariance.  With the factors of pass K and e_1, e_2 the unit vectors of the two slopes: xu1 = Solve_Mu(e_1), xu2 =
 * Solve_Mu(e_2), ss = s*s in double,
 *   Vaa = xu1[1]/ss,  Vab = xu1[2]/ss,  Vbb = xu2[2]/ss;     Vcc, Vcd, Vdd from Mv the same way.
 * With weights 1/variance the inverse of the normal matrix IS the covariance of the coefficients (for K > 0 that of the last
 * pass's weights taken as given).  The u and the v fit are treated as independent: the rho of flow2d_subset_uncertainty_2d is
 * not propagated, and neither is the correlation between overlapping subsets of neighbouring nodes.
 * Standard deviations, in double, each the square root of a variance, cast to float once:
 *   sigma_ux = sqrt(Vaa),  sigma_uy = sqrt(Vbb),  sigma_vx = sqrt(Vcc),  sigma_vy = sqrt(Vdd),
 *   sigma_divergence = sqrt(Vaa + Vdd),   sigma_vorticity = sqrt(Vbb + Vcc),
 *   measure == FLOW2D_STRAIN_SMALL:  sigma_exx = sqrt(Vaa),  sigma_eyy = sqrt(Vdd),  sigma_exy = sqrt(0.25*(Vbb + Vcc));
 *   measure == FLOW2D_STRAIN_GREEN_LAGRANGE, to first order through the Jacobian of that measure's formulas, with
 *   ja = 1.0 + a and jd = 1.0 + d:
 *     sigma_exx = sqrt((ja*ja)*Vaa + (c*c)*Vcc),     sigma_eyy = sqrt((b*b)*Vbb + (jd*jd)*Vdd),
 *     Qu = ((b*b)*Vaa + (2.0*(b*ja))*Vab) + (ja*ja)*Vbb,     Qv = ((jd*jd)*Vcc + (2.0*(jd*c))*Vcd) + (c*c)*Vdd,
 *     sigma_exy = sqrt(0.25*(Qu + Qv)).
 * Outputs in addition.  `sigmas` (a HOST struct of nine device pointers, may be NULL, each may be NULL): planes on the node grid
 * like those of `out`, NaN (0x7FC00000) at an invalid node.  `diagnostics` as in flow2d_node_strain_robust_2d, with residual and
 * centre now in sigmas (square roots of r2 as defined here).  A sigma plane or a diagnostic plane alone is output enough.
 * stats[b]: the record of flow2d_node_strain_robust_2d, reserved[0 .. 5] with its meanings, and reserved[6] = the nodes of the
 * grid that are usable but not weighable (they are among the *centre* nodes of reserved[0]); the rest 0.  The same two ordered
 * launches with slabs of flow2d_node_strain_weighted_workspace_bytes: the same bytes alone, in a lock-step batch and under graph
 * replay.
 * What follows from the text: (a) with both sigma planes 1.0f everywhere, sigma_floor = 0 and T = 0 every weight is 1.0, and the
 * nine planes of `out` and every word of the record but reserved[3 .. 6] are flow2d_node_strain_2d's; (b) with T = 0, doubling
 * both sigma planes and sigma_floor scales every sum by the power of two 1/4, so -- short of overflow and underflow -- `out`
 * does not change by a bit and every sigma plane doubles exactly.
 * FLOW2D_ERR_INVALID_ARGUMENT, and nothing written, for what flow2d_node_strain_robust_2d refuses apart from its sigma (a sigma
 * plane counts as a requested plane), for a null node_sigma_u or node_sigma_v or one that breaks the plane rules, a sigma_floor or
 * threshold that is not finite or < 0, iterations outside their limits or > 0 with T = 0, or a written range that overlaps a
 * sigma input; FLOW2D_ERR_UNSUPPORTED for 2^31 nodes or more. */
typedef struct flow2d_strain_sigma_planes {
    float* sigma_ux; /* standard deviations of the four gradients, 1 (pixels per pixel) */
    float* sigma_uy;
    float* sigma_vx;
    float* sigma_vy;
    float* sigma_divergence;
    float* sigma_vorticity;
    float* sigma_exx; /* of the chosen measure's strains */
    float* sigma_eyy;
    float* sigma_exy;
} flow2d_strain_sigma_planes;
/* Workspace bytes flow2d_node_strain_weighted_2d needs for `instances` lock-step instances of an nw x nh grid when it writes
 * statistics (0 for a zero size; a multiple of 16).  Host logic only, needs no device. */
FLOW2D_API size_t flow2d_node_strain_weighted_workspace_bytes(size_t nw, size_t nh, size_t instances);
FLOW2D_API int flow2d_node_strain_weighted_2d(flow2d_context* ctx, const float* node_u, const float* node_v,
                                              const float* node_state /* may be NULL */, const float* node_sigma_u,
                                              const float* node_sigma_v, size_t nw, size_t nh, size_t node_pitch_bytes, int spacing,
                                              int window, int order, int min_nodes, int min_state, int measure, float sigma_floor,
                                              float threshold, int iterations,
                                              const flow2d_deformation_planes* out /* host, may be NULL */,
                                              const flow2d_node_strain_diagnostics* diagnostics /* host, may be NULL */,
                                              const flow2d_strain_sigma_planes* sigmas /* host, may be NULL */,
                                              flow2d_deformation_stats* stats /* device, may be NULL */, void* workspace,
                                              size_t workspace_bytes);

/* The composition of two node fields of a sequence whose reference frame has moved (incremental DIC), out of place.  The *base* A
 * is frame 0 -> frame r at the nodes of frame 0; the *increment* B is frame r -> frame k on the same grid laid in frame r.  The
 * result is frame 0 -> frame k at the nodes of frame 0: B sampled where A carries each node, and the two deformation gradients
 * multiplied.  Added to ABI version 1 without changing any existing entry.
 * Inputs.  base[0 .. 6] and increment[0 .. 6]: HOST arrays of seven device pointers each, the planes u, v, ux, uy, vx, vy and
 * state (the outputs of the subset refinement's entries, of flow2d_predict_nodes_2d or of an earlier call of this entry), nw x nh
 * floats with node_pitch_bytes per row; increment_score (may be NULL), B's score plane; r = grid_radius
 * (1 .. FLOW2D_CORRELATION_MAX_RADIUS) and s = spacing (1 .. FLOW2D_CORRELATION_MAX_SPACING) of the grid, whose node (i, j) is
 * centred on pixel (r + i*s, r + j*s); min_state (0 or 1).  nw >= 2 and nh >= 2.
 * Everything below is IEEE double (an input is converted first, which is exact; r, s, nw, nh, i and j too); every operation is
 * rounded on its own, no fused multiply-add; division correctly rounded.  Every test is written as a positive comparison, so that
 * a NaN fails it.
 * Usable.  A node of A or of B is *usable* as in flow2d_predict_nodes_2d: state >= (float)min_state and its u, v, ux, uy, vx and
 * vy all finite.
 * No base.  A's node (i, j) is not usable.
 * Position.  Otherwise X = (r + i*s) + uA,  Y = (r + j*s) + vA (the bracket is exact),  a = (X - r)/s,  b = (Y - r)/s.  The node is
 * *outside* unless a >= -0.5, a <= nw - 0.5, b >= -0.5 and b <= nh - 0.5.
 * Cell.  i0 = floor(a) clamped to [0, nw - 2],  tx = a - i0 clamped to [0, 1] (below 0: 0; above 1: 1);  j0 and ty likewise from
 * b and nh.  Corner n = 0, 1, 2, 3 is node (i0 + di, j0 + dj) with (di, dj) = (0,0), (1,0), (0,1), (1,1) and has the weight
 *   w_n = (di ? tx : 1 - tx) * (dj ? ty : 1 - ty).
 * Only the corners that are usable in B count.  Every sum below starts from 0 and adds the terms of the usable corners in the
 * order of n.  W = sum of w_n.  The node has *no increment* when !(W > 0).
 * Sampling B.  With dx = X - (r + (i0 + di)*s) and dy = Y - (r + (j0 + dj)*s), corner n offers
 *   cu_n = (u_n + ux_n*dx) + uy_n*dy;   cv_n = (v_n + vx_n*dx) + vy_n*dy;   ux_n, uy_n, vx_n, vy_n as they are
 * (its first-order extrapolation to (X, Y): with the clamped weights it makes sampling up to half a cell beyond the grid's hull
 * safe, and dropping lost corners never divides by a sum of weights of both signs).  Each of the six values of B is
 *   (sum of w_n*c_n) / W,   each product rounded;   and with a score  scoreB = (sum of w_n*score_n) / W.
 * Composition, F = F_B * F_A, each result cast to float once:
 *   u = uA + uB;   v = vA + vB;
 *   ux = (((1 + uxB)*(1 + uxA)) + uyB*vxA) - 1;      uy = (1 + uxB)*uyA + uyB*(1 + vyA);
 *   vx = vxB*(1 + uxA) + (1 + vyB)*vxA;              vy = ((vxB*uyA) + (1 + vyB)*(1 + vyA)) - 1;
 * out_score = (float)scoreB.  out_state = FLOW2D_SUBSET_STATE_COMPOSED (66): usable at either min_state, like 65.  (A value too
 * large for a float becomes an infinity, and the node is then not usable to whoever reads it; a result that is a NaN -- a NaN score
 * of a usable corner, infinities that cancel -- is stored as 0x7FC00000.)
 * A node with no base, outside or with no increment gets NaN (0x7FC00000) in the six planes and the score, and out_state = -1.
 * Outputs.  out[0 .. 5]: HOST array of six device pointers, u, v, ux, uy, vx, vy; out_state (may be NULL); out_score (given exactly
 * when increment_score is).  Record.  record[b] (DEVICE memory, may be NULL), 64 bytes: nodes (nw * nh); composed; no_base;
 * outside; no_increment; three reserved words, written as 0.  Integers, added by integer atomics after the entry has zeroed the
 * record on the stream: alone, in a batch and in a replayed graph the same bytes.
 * Row padding and the containers beyond nw x nh are neither read into a result nor written.  One launch on the context's stream
 * (and a 64-byte memset per instance with a record); no allocation, no synchronisation (graph-capturable).  Honours
 * flow2d_context_set_batch: every plane of instance b at b * stride floats, record + b.
 * FLOW2D_ERR_INVALID_ARGUMENT, and nothing written, for a null array, a null input plane or a null one of the six output planes, a
 * zero size, nw < 2 or nh < 2, a bad pitch, a grid_radius, spacing or min_state outside its limits, a score input without a score
 * output or the reverse, a misaligned record (8), or a written range -- outputs, state, score, records, over every instance of a
 * batch -- that overlaps an input or another written range; FLOW2D_ERR_UNSUPPORTED for 2^31 nodes or more. */
#define FLOW2D_SUBSET_STATE_COMPOSED 66
typedef struct flow2d_compose_record {
    unsigned long long nodes;        /* nw * nh */
    unsigned long long composed;     /* nodes that got a composed value: state 66 */
    unsigned long long no_base;      /* the base's node is not usable: NaN, state -1 */
    unsigned long long outside;      /* carried more than half a cell beyond the grid: NaN, state -1 */
    unsigned long long no_increment; /* no usable corner with a positive weight: NaN, state -1 */
    unsigned long long reserved[3];  /* 0 */
} flow2d_compose_record;

#define FLOW2D_COMPOSE_RECORD_BYTES 64
#ifdef __cplusplus
static_assert(sizeof(flow2d_compose_record) == FLOW2D_COMPOSE_RECORD_BYTES, "flow2d_compose_record layout");
#else
_Static_assert(sizeof(flow2d_compose_record) == FLOW2D_COMPOSE_RECORD_BYTES, "flow2d_compose_record layout");
#endif

FLOW2D_API int flow2d_compose_nodes_2d(flow2d_context* ctx, const float* const* base /* u, v, ux, uy, vx, vy, state */,
                                       const float* const* increment /* the same seven */,
                                       const float* increment_score /* may be NULL */, size_t nw, size_t nh, size_t node_pitch_bytes,
                                       int grid_radius, int spacing, int min_state, float* const* out /* u, v, ux, uy, vx, vy */,
                                       float* out_state /* may be NULL */, float* out_score /* with increment_score */,
                                       flow2d_compose_record* record /* device, may be NULL */);

/* The flow of the previous pyramid level resampled to this level's size (the bits of flow2d_resample_xy_pair into out_u / out_v)
 * and frame_1 warped by it (the bits of flow2d_registration_2d into `output`) in one launch: replaces the
 * CudaOperationResample2D::Execute + CudaOperationRegistration2D::Execute pair of optical_flow_2d.cpp:314-362 at every
 * level; at the coarsest one -- flow_u = flow_v = NULL, in_width = in_height = 0 -- out_u = out_v = 0 over width x height (the two
 * whole-plane memsets of optical_flow_2d.cpp:308-313) and frame_1 warped by that.  Written planes must be distinct from each other
 * and from every plane read. */
FLOW2D_API int flow2d_upsample_registration_2d(flow2d_context* ctx, const float* flow_u, const float* flow_v, size_t in_width,
                                               size_t in_height, float* out_u, float* out_v, const float* frame_0,
                                               const float* frame_1, size_t width, size_t height, size_t pitch_bytes, float hx,
                                               float hy, float* output);
/* The same at an exactly doubled level (width = 2 in_width, height = 2 in_height; anything else FLOW2D_ERR_UNSUPPORTED) with
 * out_u / out_v kept at in_width x in_height.  At such a level the resampled flow is a replication: each 2 x 2 block of pixels
 * holds one input pixel's value after the resample's four multiplications (not the identity: -0 becomes +0, denormals round).
 * out[y][x] is that value, i.e. what flow2d_upsample_registration_2d stores at (2y .. 2y + 1, 2x .. 2x + 1); `output` is that
 * entry's warped frame bit for bit.  Readers of the level index the planes with (y >> 1, x >> 1): flow2d_solve_level with
 * base_flow_shift = 1, flow2d_add_median_2d_pair_half.  No written byte range may meet a read one or another written one, over
 * every instance of a batch (FLOW2D_ERR_INVALID_ARGUMENT). */
FLOW2D_API int flow2d_upsample_registration_half_2d(flow2d_context* ctx, const float* flow_u, const float* flow_v, size_t in_width,
                                                    size_t in_height, float* out_u, float* out_v, const float* frame_0,
                                                    const float* frame_1, size_t width, size_t height, size_t pitch_bytes,
                                                    float hx, float hy, float* output);
/* launches of flow2d_upsample_registration_half_2d queued by this process so far: tells which path a pyramid took (the host
 * layer takes it at every level that is exactly twice the previous one and solved by the strips) */
FLOW2D_API unsigned long long flow2d_half_base_flow_launches(void);

/* The first level of a pyramid that starts from a prior flow instead of from zero (no reference counterpart): the counterpart of
 * flow2d_upsample_registration_2d with a full-resolution prior in place of the previous level's flow, in one launch; added to ABI
 * version 1 without changing any existing entry.  prior_u / prior_v are in_width x in_height planes holding a flow in
 * full-resolution pixels; frame_0 / frame_1 are the level's frames, width x height, width <= in_width and height <= in_height
 * (equal sizes: the prior enters at level 0).  All planes share pitch_bytes.  fp32, every operation rounded on its own, no fused
 * multiply-add:
 *   Sanitising.  A prior pixel where u or v is not finite (NaN, +Inf, -Inf) counts as (0, 0) -- the vector the unseeded pyramid
 *     starts from -- in BOTH planes, and is counted once in the record, whether or not an output's cells reach it.
 *   Resample.  The sanitised planes are brought to width x height exactly as flow2d_resample_xy_pair does it (resample_2d.cu:34-118):
 *     per output the x pass over the cells of every prior row its y cells touch -- cells summed left to right from 0, the first and
 *     the last with their fractions, the sum times width / (float)in_width, rounded to float like the temp plane of the two-launch
 *     form --, then the y pass over those values, times height / (float)in_height.  No magnitude scaling: the vectors stay in
 *     full-resolution pixels and the level's hx / hy carry the units, as everywhere in the pyramid.  The result goes to out_u / out_v.
 *   Registration.  `output` is exactly what flow2d_registration_2d gives for frame_0, frame_1, out_u, out_v, hx, hy
 *     (registration_2d.cu:34-73: a vector that leaves the frame, or a NaN position, takes frame_0's pixel).
 * Record.  record[b] (DEVICE memory, 8-byte aligned, one unsigned long long per instance of a lock-step batch) gets the number of
 * prior pixels of instance b that were not finite.  An integer, added by integer atomics after the entry has zeroed the record on
 * the stream: repeated calls, a replayed graph and an instance alone or in its batch give the same bytes.
 * Row padding and the containers beyond in_width x in_height and width x height are neither read into a result nor written.  One
 * launch on the context's stream (and an 8-byte memset per instance); no allocation, no synchronisation, no host round trip
 * (graph-capturable).  Honours flow2d_context_set_batch: every plane of instance b at b * stride floats, record + b.  Per-lane
 * offsets are 32-bit while in_height * pitch_bytes fits them, else 64-bit.
 * FLOW2D_ERR_INVALID_ARGUMENT, before any launch, for a null plane or record (or a misaligned one), a zero size, a level larger than
 * the prior in either direction, a bad pitch (the rule of flow2d_consistency_2d), an hx or hy that is not finite and > 0, or a
 * written byte range -- out_u, out_v, output, the records -- that meets a read one or another written one, over every instance of
 * a batch. */
FLOW2D_API int flow2d_prior_registration_2d(flow2d_context* ctx, const float* prior_u, const float* prior_v, size_t in_width,
                                            size_t in_height, float* out_u, float* out_v, const float* frame_0, const float* frame_1,
                                            size_t width, size_t height, size_t pitch_bytes, float hx, float hy, float* output,
                                            unsigned long long* record /* device */);

/* A flow carried along itself onto the next frame's grid (no reference counterpart; added to ABI version 1 without changing any
 * existing entry): the prior of a warm-started sequence.  (flow_u, flow_v) is the flow of the pair (k, k + 1) on frame k's grid; the
 * content of pixel p has moved to p + step * flow(p), and that is where the vector belongs on frame k + 1's grid.  A deterministic
 * forward splat; fp32, every operation rounded on its own, no fused multiply-add.  All planes are width x height with pitch_bytes.
 * For the source pixel p = (x, y) with index i = y * width + x (width * height <= 2^32 - 1):
 *   usable    u = flow_u[p] and v = flow_v[p] are finite, and mask == NULL or mask[p] == 0 (a NaN in the mask: not usable).
 *             Otherwise p is counted in `unusable` and takes no further part.
 *   landing   lx = (float)x + step * u,  ly = (float)y + step * v
 *   target    tx = floorf(lx + 0.5f),  ty = floorf(ly + 0.5f);  unless 0 <= tx <= width - 1 and 0 <= ty <= height - 1 -- compared
 *             as floats, so that a NaN or an infinity fails and no such value is converted to an integer -- p is counted in `left`.
 *             Otherwise p is counted in `landed`.
 *   distance  ex = lx - tx, ey = ly - ty, d2 = ex*ex + ey*ey, dq = min((unsigned)(d2 * 4194304.0f), 0x7FFFFF)
 *   match     with frame_from and frame_to and photo_scale != 0:  g = S(frame_to, (min(max(lx, 0), width - 1), min(max(ly, 0),
 *             height - 1))), S the bilinear sample of flow2d_consistency_2d;  diff = fabsf(frame_from[p] - g) * photo_scale;
 *             q = 255 when diff is not finite, else min(255, (unsigned)diff).  Without frames or with photo_scale == 0: q = 0.
 *   key       (u64)(255 - q) << 56 | (u64)(0x7FFFFF - dq) << 32 | (u64)(0xFFFFFFFF - i)       (never zero: i <= 2^32 - 2)
 * Every target keeps the LARGEST key offered to it (one 64-bit integer atomic max per landed pixel on a word of the workspace,
 * which the entry zeroes on the stream first; max commutes, so the winner depends on no arrival order): the candidate that matches
 * photometrically best, then the one that lands nearest to the pixel's centre, then the one with the lowest source index.
 * Resolve.  A target takes its winner's (u, v) bit for bit -- the vector is NOT scaled by step --; a target without a winner is a
 * hole, counted in `holes`, and holds the quiet NaN 0x7fc00000 in both planes.
 * Fill.  fill_passes (0 .. FLOW2D_PROPAGATE_MAX_FILL) passes, each over the result of the one before: a pixel that is not finite in
 * both components and has, among its eight neighbours inside the frame, at least one that is, takes the mean of those -- per
 * component the sum from 0 in the order (-1,-1), (0,-1), (1,-1), (-1,0), (1,0), (-1,1), (0,1), (1,1), divided by the count as a
 * float -- and is counted in `filled`; every other pixel is copied.  The pixels still not finite after the last pass (the holes,
 * when fill_passes == 0) are counted in `unfilled`.  The passes ping-pong between out_u / out_v and two planes of the workspace;
 * the last one writes out_u / out_v.
 * Record.  record (DEVICE memory, 8-byte aligned, NULL: no counts) gets per instance b of a lock-step batch, at record +
 * 8 * b, eight unsigned long long: pixels (= width * height = unusable + left + landed), unusable, left, landed, holes, filled,
 * unfilled, and a reserved zero.  Integers, summed per wave and added by integer atomics after the entry has zeroed the record on
 * the stream: repeated calls, a replayed graph and an instance alone or in its batch give the same bytes.
 * `workspace` (16-byte aligned) holds at least flow2d_propagate_flow_workspace_bytes(width, height, instances) bytes (instances =
 * the batch count): 16 bytes per pixel and instance -- the keys of all instances first, then two dense planes per instance.
 * 2 + fill_passes launches and two memsets on the context's stream; no allocation, no synchronisation, no host round trip
 * (graph-capturable).  Honours flow2d_context_set_batch: every plane of instance b at b * stride floats.  Per-lane offsets are
 * 32-bit while height * pitch_bytes fits them, else 64-bit.  Row padding is read only as the unselected half of a column pair and
 * never written.
 * FLOW2D_ERR_INVALID_ARGUMENT, before any launch, for a null flow or output plane, a zero size, width * height > 2^32 - 1, a bad
 * pitch (the rule of flow2d_consistency_2d), one frame without the other, a step that is not finite or is zero, a photo_scale that
 * is not finite or is negative, fill_passes out of range, a null or misaligned workspace, a misaligned record, or a written byte
 * range -- out_u, out_v, the records, the workspace -- that meets a read one or another written one, over every instance of a
 * batch. */
#define FLOW2D_PROPAGATE_MAX_FILL 64
#define FLOW2D_PROPAGATE_RECORD_BYTES 64
typedef struct flow2d_propagate_record { /* the eight counts of one instance, as they lie in `record` */
    unsigned long long pixels, unusable, left, landed, holes, filled, unfilled, reserved;
} flow2d_propagate_record;
#ifdef __cplusplus
static_assert(sizeof(flow2d_propagate_record) == FLOW2D_PROPAGATE_RECORD_BYTES, "flow2d_propagate_record layout");
#else
_Static_assert(sizeof(flow2d_propagate_record) == FLOW2D_PROPAGATE_RECORD_BYTES, "flow2d_propagate_record layout");
#endif
/* Host logic only, needs no device; 0 for a zero size. */
FLOW2D_API size_t flow2d_propagate_flow_workspace_bytes(size_t width, size_t height, size_t instances);
FLOW2D_API int flow2d_propagate_flow_2d(flow2d_context* ctx, const float* flow_u, const float* flow_v, const float* mask,
                                        const float* frame_from, const float* frame_to, size_t width, size_t height,
                                        size_t pitch_bytes, float step, float photo_scale, int fill_passes, float* out_u,
                                        float* out_v, unsigned long long* record /* device */, void* workspace);

/* resample_x / resample_y (src/kernels/resample_2d.cu:34-75,77-118): area-weighted 1-D resample. */
FLOW2D_API int flow2d_resample_x(flow2d_context* ctx, const float* input, float* output, size_t out_width,
                                 size_t out_height, size_t in_width, size_t pitch_bytes);
FLOW2D_API int flow2d_resample_y(flow2d_context* ctx, const float* input, float* output, size_t out_width,
                                 size_t out_height, size_t in_height, size_t pitch_bytes);

/* Two-plane forms of the three launchers the pyramid calls once for u and once for v (or once per frame) with
 * identical geometry: one launch does what two calls of the single-plane entry do, plane set `a` and plane set
 * `b` independently and with the same results (the second set rides in grid.z).  They replace the back-to-back
 * launch pairs of optical_flow_2d.cpp:284-303 (frames), :314-338 (flow resample), :480-500 (add), :505-530 (median);
 * on the coarse levels a launch costs more than its work.  The four output planes must be distinct. */
FLOW2D_API int flow2d_add_2d_pair(flow2d_context* ctx, float* operand_0_a, const float* operand_1_a,
                                  float* operand_0_b, const float* operand_1_b, size_t width, size_t height,
                                  size_t pitch_bytes);
FLOW2D_API int flow2d_median_2d_pair(flow2d_context* ctx, const float* input_a, const float* input_b, size_t width,
                                     size_t height, size_t pitch_bytes, size_t window, float* output_a,
                                     float* output_b);
/* add_2d followed by median_2d (optical_flow_2d.cpp:480-530: u += du, then the median of u) in one launch: the filter runs
 * over input + addend, formed per pixel as it is read -- add_2d's sum is one rounded addition (add_2d.cu:33-46), so the
 * result is the same -- and the plane of sums is neither written nor read back.  input is NOT modified.  input_b,
 * addend_b, output_b: optional second plane set (all three or none). */
FLOW2D_API int flow2d_add_median_2d_pair(flow2d_context* ctx, const float* input_a, const float* addend_a,
                                         const float* input_b, const float* addend_b, size_t width, size_t height,
                                         size_t pitch_bytes, size_t window, float* output_a, float* output_b);
/* flow2d_add_median_2d_pair with the INPUT planes held at half the size in both directions, (height + 1) / 2 rows of
 * (width + 1) / 2 pixels in the same pitch: pixel (y, x) of the sum is input[y >> 1][x >> 1] + addend[y][x], the borders mirrored
 * before the shift.  What that entry returns for the input replicated to width x height, bit for bit (NaN and -0 windows
 * included), without the replicated planes: the median after an exactly doubled pyramid level, whose base flow
 * flow2d_upsample_registration_half_2d left at the previous level's size.  No output byte range may meet an input's or an
 * addend's, over every instance of a batch (FLOW2D_ERR_INVALID_ARGUMENT). */
FLOW2D_API int flow2d_add_median_2d_pair_half(flow2d_context* ctx, const float* input_a, const float* addend_a,
                                              const float* input_b, const float* addend_b, size_t width, size_t height,
                                              size_t pitch_bytes, size_t window, float* output_a, float* output_b);
FLOW2D_API int flow2d_resample_x_pair(flow2d_context* ctx, const float* input_a, float* output_a,
                                      const float* input_b, float* output_b, size_t out_width, size_t out_height,
                                      size_t in_width, size_t pitch_bytes);
FLOW2D_API int flow2d_resample_y_pair(flow2d_context* ctx, const float* input_a, float* output_a,
                                      const float* input_b, float* output_b, size_t out_width, size_t out_height,
                                      size_t in_height, size_t pitch_bytes);

/* resample_x into a temp plane followed by resample_y (CudaOperationResample2D::Execute,
 * src/cuda_operations/2d/cuda_operation_resample_2d.cpp:99-152) as ONE launch without the temp plane: every output evaluates
 * the x pass for the input rows of its y cells (same cell sums, rounded to float like the temp) and then the y pass.
 * Bit-identical to the two calls; meant for up-sampling (the flow of the previous pyramid level: one or two cells per
 * direction), correct for any ratio.  input_b / output_b: optional second plane (both or neither). */
FLOW2D_API int flow2d_resample_xy_pair(flow2d_context* ctx, const float* input_a, float* output_a, const float* input_b,
                                       float* output_b, size_t in_width, size_t in_height, size_t out_width,
                                       size_t out_height, size_t pitch_bytes);

/* The x pass of resample_2d.cu:34-75 for SEVERAL output widths in one trip over the input.  The reference resamples
 * both frames from full resolution at every pyramid level (optical_flow_2d.cpp:284-303), i.e. reads each frame once per
 * level; here every input row is read once, kept in LDS, and the x-resampled rows of all `level_count` widths are written
 * side by side into one "packed" plane: level l occupies columns [column_offsets[l], column_offsets[l] + out_widths[l])
 * of every row (offsets in floats, multiples of 4, segments disjoint, all within the pitch).  Each output is the same
 * left-to-right cell sum as flow2d_resample_x produces for that width (bit-identical).  The y pass of a level is then
 * flow2d_resample_y on `packed + column_offsets[l]`.  input_b / packed_b: optional second plane (both or neither).
 * Needs in_width <= 15360 (a row lives in LDS); FLOW2D_ERR_UNSUPPORTED beyond, or for more than 16 levels. */
#define FLOW2D_RESAMPLE_MAX_LEVELS 16
FLOW2D_API int flow2d_resample_x_levels(flow2d_context* ctx, const float* input_a, float* packed_a, const float* input_b,
                                        float* packed_b, size_t in_width, size_t height, size_t pitch_bytes,
                                        size_t level_count, const size_t* out_widths, const size_t* column_offsets);

/* The y passes of resample_2d.cu:77-118 for SEVERAL levels in one launch, the counterpart of flow2d_resample_x_levels: level l
 * reads columns [column_offsets[l], column_offsets[l] + out_widths[l]) of the packed plane (in_height rows) and writes an
 * out_widths[l] x out_heights[l] plane region whose first row is row output_rows[l] of the output plane (regions disjoint;
 * the region of a level is a plane of its own: pointer = output + output_rows[l] * pitch).  Each output is the same top-to-bottom
 * cell sum as flow2d_resample_y produces for that level (bit-identical).  packed_b / output_b: optional second plane. */
FLOW2D_API int flow2d_resample_y_levels(flow2d_context* ctx, const float* packed_a, float* output_a, const float* packed_b,
                                        float* output_b, size_t in_height, size_t pitch_bytes, size_t level_count,
                                        const size_t* out_widths, const size_t* out_heights, const size_t* column_offsets,
                                        const size_t* output_rows);

/* flow2d_resample_x_levels followed by flow2d_resample_y_levels as ONE launch that never stores the x-resampled rows: every source
 * row is read once and only the levels are written.  Level l becomes an out_widths[l] x out_heights[l] region of the output plane
 * whose first row is output_rows[l] and whose first column is output_columns[l] (in floats, a multiple of 4; output_columns may be
 * NULL: every region starts at column 0).  Each output is bit-identical to the two calls composed: the left-to-right x sum
 * times 1 / R, then the top-to-bottom y sum of those values times 1 / R.
 * Eligible geometry (FLOW2D_ERR_UNSUPPORTED otherwise, before anything is launched): what a halving pyramid produces -- every
 * level's ratio R is one power of two, 2 ... 256, in BOTH directions (out_widths[l] * R == in_width and out_heights[l] * R ==
 * in_height), no two levels share a ratio, in_width is a multiple of 32 and at most 8192, at most 16 levels.
 * Ranges: inputs are in_height rows of pitch_bytes (a multiple of 16, pointers 16-byte aligned); an output plane is written
 * between its first and its last region row, [output + min(output_rows) * pitch, output + max(output_rows + out_heights) * pitch),
 * and the caller owns those rows.  These byte ranges (with a batch: of all instances) must not meet each other or an input, and
 * the regions of one plane must be disjoint rectangles inside the pitch: FLOW2D_ERR_INVALID_ARGUMENT otherwise, whatever the base
 * pointers are.  input_b / output_b: optional second plane (both or neither). */
FLOW2D_API int flow2d_resample_xy_levels(flow2d_context* ctx, const float* input_a, float* output_a, const float* input_b,
                                         float* output_b, size_t in_width, size_t in_height, size_t pitch_bytes, size_t level_count,
                                         const size_t* out_widths, const size_t* out_heights, const size_t* output_rows,
                                         const size_t* output_columns);
/* How many launches flow2d_resample_xy_levels has queued in this process, all contexts together (a launch recorded into a graph
 * counts once, its replays do not): tells a caller or a test which path a pyramid took. */
FLOW2D_API unsigned long long flow2d_resample_xy_levels_launches(void);

/* compute_phi_ksi (src/kernels/solve_2d.cu:43-198). */
FLOW2D_API int flow2d_compute_phi_ksi(flow2d_context* ctx, const float* frame_0, const float* frame_1,
                                      const float* flow_u, const float* flow_v, const float* flow_du,
                                      const float* flow_dv, size_t width, size_t height, size_t pitch_bytes, float hx,
                                      float hy, float equation_smoothness, float equation_data, float* phi,
                                      float* ksi);

/* solve_2d (src/kernels/solve_2d.cu:200-377): one Jacobi sweep, brightness constancy. */
FLOW2D_API int flow2d_solve_2d(flow2d_context* ctx, const float* frame_0, const float* frame_1, const float* flow_u,
                               const float* flow_v, const float* flow_du, const float* flow_dv, const float* phi,
                               const float* ksi, size_t width, size_t height, size_t pitch_bytes, float hx, float hy,
                               float equation_alpha, float* temp_du, float* temp_dv);

/* One Jacobi sweep with the opt-in FLOW2D_CONSTANCY_GRADIENT_UNTILED data term (no reference counterpart;
 * same arguments as flow2d_solve_2d_grad). */
FLOW2D_API int flow2d_solve_2d_grad_untiled(flow2d_context* ctx, const float* frame_0, const float* frame_1,
                                            const float* flow_u, const float* flow_v, const float* flow_du,
                                            const float* flow_dv, const float* phi, const float* ksi, size_t width,
                                            size_t height, size_t pitch_bytes, float hx, float hy,
                                            float equation_alpha, float* temp_du, float* temp_dv);

/* solve_2d_grad (src/kernels/solve_2d.cu:683-952): one Jacobi sweep, gradient constancy, including
 * the reference's 16x8 block rule for the second derivatives. */
FLOW2D_API int flow2d_solve_2d_grad(flow2d_context* ctx, const float* frame_0, const float* frame_1,
                                    const float* flow_u, const float* flow_v, const float* flow_du,
                                    const float* flow_dv, const float* phi, const float* ksi, size_t width,
                                    size_t height, size_t pitch_bytes, float hx, float hy, float equation_alpha,
                                    float* temp_du, float* temp_dv);

/* solve_2d_log (src/kernels/solve_2d.cu:391-669): one Jacobi sweep on the logarithmic derivatives
 * (gradient constancy of log(I + 1)), including that kernel's block rule: every 16x8 block's halo -- of the
 * frames, u, v, du, dv, phi and ksi alike -- holds the block's own edge pixel (:448,462,476,490). */
FLOW2D_API int flow2d_solve_2d_log(flow2d_context* ctx, const float* frame_0, const float* frame_1,
                                   const float* flow_u, const float* flow_v, const float* flow_du,
                                   const float* flow_dv, const float* phi, const float* ksi, size_t width,
                                   size_t height, size_t pitch_bytes, float hx, float hy, float equation_alpha,
                                   float* temp_du, float* temp_dv);

/* out[y][x] = log(in[y][x] + 1.0f) over width x height, formed by the function every kernel of the log-derivative term
 * calls (the device library's logf).  Not a step of the flow: it hands a checker the device's own logarithms, so that a
 * CPU restatement of solve_2d_log can be held to the kernels bit for bit (a CPU's libm differs from the device library
 * in the last place).  One plane, on the context's stream; `in` and `out` share the pitch and must not overlap; nothing
 * outside width x height is written.  Not batch-aware. */
FLOW2D_API int flow2d_log_frame_2d(flow2d_context* ctx, const float* in, float* out, size_t width, size_t height,
                                   size_t pitch_bytes);

/* Opt-in red-black successive over-relaxation: ONE iteration = the pixels with even (x + y), then the odd
 * ones, relaxed in place on flow_du / flow_dv with factor omega in (0, 2).  NOT a reference kernel: the
 * reference relaxes with Jacobi sweeps, so this mode has no parity with it at equal iteration
 * counts; it exists because BASELINE.json names the scheme, and is checked against its own oracle restatement. */
FLOW2D_API int flow2d_solve_2d_sor(flow2d_context* ctx, const float* frame_0, const float* frame_1,
                                   const float* flow_u, const float* flow_v, float* flow_du, float* flow_dv,
                                   const float* phi, const float* ksi, size_t width, size_t height, size_t pitch_bytes,
                                   float hx, float hy, float equation_alpha, float omega, int data_constancy);

/* ---- the solver's fixed-point loop of one level -------------------------------------------
 * Replaces the launch loop of CudaOperationSolve2D::Execute
 * (src/cuda_operations/2d/cuda_operation_solve_2d.cpp:229-300): zero du/dv (level width x
 * container_height rows), then outer x [compute_phi_ksi, inner x (sweep, swap)].  The library
 * owns the ping-pong; *result_in_temp tells the caller which pair holds the result (0: flow_du /
 * flow_dv, 1: temp_du / temp_dv), so a host wrapper can swap its own pointers like the reference
 * does (:288-289).  No host synchronisation inside.  `algorithm`: see flow2d_solver_algorithm. */
typedef enum flow2d_solver_algorithm {
    FLOW2D_SOLVER_AUTO = 0,      /* library picks the fastest bit-exact path for the level size */
    FLOW2D_SOLVER_PER_SWEEP = 1, /* one launch per reference kernel launch (K6, K7/K9/K11) */
    FLOW2D_SOLVER_FUSED = 2,     /* phi/ksi + the inner sweeps of an outer iteration fused into ceil(inner / 5)
                                  * launches (one for inner <= 5); needs inner >= 1 */
    FLOW2D_SOLVER_SINGLE_WORKGROUP = 3, /* the whole level (all outer x inner iterations) in one launch on one
                                          CU; levels up to 64 x 64 pixels */
    FLOW2D_SOLVER_TILED = 4      /* one launch per outer iteration like FUSED, on 16x16 / 32x16 LDS tiles with a halo:
                                  * spreads small and mid-size levels over the whole chip; 1 <= inner <= 5; Grey,
                                  * Gradient and Gradient-untiled data terms */
} flow2d_solver_algorithm;

typedef struct flow2d_solve_params {
    size_t width, height;        /* level size */
    size_t pitch_bytes;          /* container pitch */
    size_t container_height;     /* rows of the full-resolution container (memset extent) */
    float hx, hy;                /* grid spacing of the level */
    float equation_alpha;
    float equation_smoothness;
    float equation_data;
    size_t outer_iterations_count;
    size_t inner_iterations_count;
    int data_constancy;          /* flow2d_constancy */
    int algorithm;               /* flow2d_solver_algorithm */
    float sor_omega;             /* 0 (default): Jacobi sweeps as in the reference.  In (0, 2): every inner iteration
                                    is one red-black SOR iteration instead (opt-in, no reference parity).  AUTO runs it
                                    temporally blocked -- LDS tiles or strips by level size, two iterations per launch --,
                                    FUSED / TILED (at most two iterations per outer iteration) ask for one of the two,
                                    PER_SWEEP for two half-sweep launches per iteration, in place; SINGLE_WORKGROUP and
                                    the LogDerivatives term have no red-black form (FLOW2D_ERR_UNSUPPORTED). */
    int base_flow_shift;         /* 0 (default): flow_u / flow_v are width x height planes.  1: they are held at half the size
                                    in both directions -- pixel (y, x) reads them at (y >> 1, x >> 1), same pitch -- as
                                    flow2d_upsample_registration_half_2d leaves them; the same result as with the replicated
                                    planes, bit for bit.  With the strips only (algorithm resolves to FLOW2D_SOLVER_FUSED);
                                    anything else, or another value, FLOW2D_ERR_UNSUPPORTED before any launch. */
} flow2d_solve_params;

/* Which algorithm flow2d_solve_level runs for a request: `requested` resolved (AUTO -> one of the four), or -1 when the
 * requested algorithm cannot run the level (SINGLE_WORKGROUP above 64 x 64; FUSED without sweeps, or on planes of
 * 4 GiB and more, which its 32-bit buffer offsets cannot address -- AUTO takes the per-sweep kernels there; TILED with
 * more than 5 sweeps or the LogDerivatives term).  Host logic only, needs no device. */
FLOW2D_API int flow2d_solver_algorithm_for(int requested, size_t width, size_t height, size_t pitch_bytes,
                                           size_t outer_iterations_count, size_t inner_iterations_count,
                                           int data_constancy);

FLOW2D_API int flow2d_solve_level(flow2d_context* ctx, const float* frame_0, const float* frame_1,
                                  const float* flow_u, const float* flow_v, float* flow_du, float* flow_dv,
                                  float* phi, float* ksi, float* temp_du, float* temp_dv,
                                  const flow2d_solve_params* params, int* result_in_temp);

/* Whether flow2d_solve_level runs these parameters with base_flow_shift = 1 (the field itself is not looked at): 1 when the level
 * resolves to the strips on this context -- AUTO gives a lock-step group fewer levels to the tiles, so the context's group
 * counts --, 0 otherwise.  Host logic only: the same answer for an eager run and while a graph is recorded. */
FLOW2D_API int flow2d_solve_level_takes_half_base(flow2d_context* ctx, const flow2d_solve_params* params);

/* ---- launch timing of the solver (measurement only; bench.py's roofline leg) ----------------
 * mode 1: every flow2d_solve_level call is bracketed by a pair of events on the context's stream
 * (the reference's own per-level timer, cuda_operation_solve_2d.cpp:220,302).  mode 2: additionally
 * every launch of the level's dominant kernel (the Jacobi sweep, or the fused outer-iteration kernel)
 * is bracketed by its own event pair.  Nothing synchronises; read the records after
 * flow2d_synchronize.  mode 0 switches the collection off. */
typedef struct flow2d_timing_record {
    size_t width, height;
    size_t outer, inner;
    int data_constancy;
    int algorithm;          /* the algorithm actually used (flow2d_solver_algorithm, never AUTO) */
    int kernel_launches;    /* launches of the dominant solver kernel inside the bracket */
    float elapsed_ms;       /* event time of the whole solve call */
    float kernel_ms;        /* mode 2: sum of the dominant kernel's launch durations; -1 otherwise */
    double algorithmic_bytes_per_launch; /* W*H*40 per sweep launch, W*H*(32+40*inner)/ceil(inner/5) per fused launch */
} flow2d_timing_record;

/* Diagnostics of the fused kernel (FLOW2D_SOLVER_FUSED): its sweeps divide through a reciprocal prepared once per pixel
 * and outer iteration (three instructions instead of the eleven of a correctly rounded division; bit-identical for all
 * operands inside the normal range, proven by exhaustion over all significand pairs), and a wavefront that meets
 * operands outside that range -- a denominator outside [2^-30, 2^40], a non-zero numerator below 2^-80, an infinite or
 * NaN result -- repeats its strip with the plain division.  Number of such repeats on this context since it was
 * created (synchronises the stream). */
FLOW2D_API int flow2d_fused_fallbacks(flow2d_context* ctx, unsigned long long* waves);
/* Waves of launches that never tried the short forms because the level's grid spacing lies outside the range they are
 * proven for (2h or 4h outside [2^-30, 2^40], a NaN spacing): such a launch runs the plain expressions throughout.  Counted
 * apart from the guard trips above (synchronises the stream). */
FLOW2D_API int flow2d_fused_plain_waves(flow2d_context* ctx, unsigned long long* waves);
/* The shader clock the device holds while other work runs.  flow2d_clock_probe_start queues, on this context's stream, one
 * sleeping wave per XCD that brackets `duration_us` microseconds with the constant 100 MHz clock and the shader clock (it takes
 * no issue slots from the kernels it runs beside: queue it on a context of its own while the work of interest runs on others);
 * flow2d_clock_probe_read waits for it and returns cycles / time per XCD in GHz (0 for an XCD no wave landed on).  Why it matters:
 * the chip's power management moves the clock between about 1.6 and 2.4 GHz with the power the running kernels draw -- the strip
 * kernel's instruction stream takes 13-16 % longer beside its own HBM traffic than on cache-resident rows AT THE SAME CYCLE COUNT,
 * and the eight XCDs of one chip differ by 3-5 % -- so a launch duration is only comparable at a known clock. */
FLOW2D_API int flow2d_clock_probe_start(flow2d_context* ctx, double duration_us);
FLOW2D_API int flow2d_clock_probe_read(flow2d_context* ctx, double* ghz_per_xcd);
/* The blocks a strip launch of a width x height level with `inner` sweeps and `instances` lock-step instances runs on this
 * device, in launch order: out[4 i .. 4 i + 3] = block column, strip, first row, end row of launch block i (all -1 for an id the
 * plan leaves empty); *grid_blocks = the launch's grid (a multiple of eight: workgroups are dealt to the eight XCDs in turn and
 * every XCD gets a contiguous, equally heavy run of the plan).  FLOW2D_ERR_INVALID_ARGUMENT when capacity_blocks is too small
 * (*grid_blocks is set).  A test hook: the order must be a permutation of the plan, the strips a partition of the level. */
FLOW2D_API int flow2d_fused_block_order(flow2d_context* ctx, size_t width, size_t height, size_t inner, size_t instances,
                                        int* out, size_t capacity_blocks, size_t* grid_blocks);
/* The same for a device of `cus` compute units (1 ... FLOW2D_PLANNING_CUS_MAX), without a context or a device: what
 * flow2d_fused_block_order answers on a context after flow2d_context_set_planning_cus(ctx, cus) (it reflects the planning
 * count).  flow2d_fused_plan_for_cus gives the plan itself: plan[0 .. 4] = rows of an interior strip, rows of a strip on the
 * first or last row of strips (equal: uniform strips; different: a border-aware plan, whose first and last block column are cut
 * into strips of the second height throughout), strips per interior block column, block columns, blocks of the launch (per
 * instance); *side_blocks (may be null) = the blocks of the first and last block column when the launch order deals them over
 * the eight runs, 0 when it leaves them at the end of the order or the plan is uniform.  `instances` is what shares the launch:
 * a lock-step group whose single-pair plan (instances = 1) has interior strips of 128 rows and more is launched instance by
 * instance with that plan.  Added to ABI version 1 without changing any existing entry; test hooks like the entry above. */
FLOW2D_API int flow2d_fused_block_order_for_cus(int cus, size_t width, size_t height, size_t inner, size_t instances, int* out,
                                                size_t capacity_blocks, size_t* grid_blocks);
FLOW2D_API int flow2d_fused_plan_for_cus(int cus, size_t width, size_t height, size_t inner, size_t instances, int* plan,
                                         int* side_blocks);
/* Rows per strip of a streaming launch on a device of `cus` compute units: kind FLOW2D_STREAM_GAUSSIAN -- flow2d_gaussian_blur
 * with a radius of 1 ... 6 (larger radii do not stream), 16 ... 128 rows -- or FLOW2D_STREAM_MEDIAN -- flow2d_median_2d and its
 * pair and add forms with radius 1, 2, 3 for the windows 3, 5, 7, 8 ... 64 rows --, for `instances` lock-step instances.  The
 * launchers take their strips from the same function.  -1 for arguments outside those ranges.  No context, no device; a test
 * hook (added to ABI version 1 without changing any existing entry). */
#define FLOW2D_STREAM_GAUSSIAN 0
#define FLOW2D_STREAM_MEDIAN 1
FLOW2D_API int flow2d_stream_rows_for_cus(int cus, int kind, size_t width, size_t height, int radius, size_t instances);
/* Strip launches queued by this process so far that the packed build of the strip kernel served: the launches of a lone context
 * (flow2d_context_set_lone) with at most one workgroup per CU whose data term, sweep count and kind the packed build holds -- a
 * launch it does not hold (the LogDerivatives term, the continued sweeps of an outer iteration) goes to the pipeline's build and
 * is not counted.  A lock-step group that shares a launch counts once.  A test hook: the two builds must give the same bits, and
 * this is what tells a test which of them it compared. */
FLOW2D_API unsigned long long flow2d_fused_packed_launches(void);

FLOW2D_API int flow2d_timing_enable(flow2d_context* ctx, int mode);
/* mode 2 brackets individual launches only for levels of at least min_width x min_height pixels
 * (default 0 x 0 = every level); smaller levels still get their mode-1 record. */
FLOW2D_API int flow2d_timing_launch_filter(flow2d_context* ctx, size_t min_width, size_t min_height);
FLOW2D_API int flow2d_timing_count(flow2d_context* ctx, size_t* count);
FLOW2D_API int flow2d_timing_get(flow2d_context* ctx, size_t index, flow2d_timing_record* out);
FLOW2D_API int flow2d_timing_reset(flow2d_context* ctx);

#ifdef __cplusplus
}
#endif

#endif /* FLOW2D_C_ABI_H_ */
