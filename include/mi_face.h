/*
 * mi_face.h — C ABI of the MI355X-native BlazeFace / face-mesh / iris inference path.
 *
 * Drop-in boundary for okieraised/rs-face-detection-tflite's three `infer` entry points and for the engine surface
 * they call into (the `tflite` crate).  Every entry point cites the reference interface it replaces; paths are
 * relative to /root/reference/src/face_detection_lite/.  Plain pointers and sizes only: no C++/torch types.
 *
 * Conventions
 *   - every function returns MI_OK (0) or a negative MI_E* code; the message is in mi_last_error() (thread-local).
 *     Nothing panics/aborts across the ABI (the reference panics at the unwrap/assert sites listed in SURVEY.md §5;
 *     here those become MI_EINVAL / MI_ERANGE returns).
 *   - `mem` says where the caller's tensor buffers live: MI_MEM_HOST (pageable/pinned host memory; the library
 *     stages through its own device buffers) or MI_MEM_DEVICE (HIP device pointers on the handle's GPU).
 *   - `stream` is a hipStream_t passed as void* (NULL = the handle's own stream).  With MI_MEM_DEVICE and a caller
 *     stream the call is asynchronous with respect to the host; with MI_MEM_HOST it returns after results landed.
 *   - handles are bound to one GPU (`device` = HIP ordinal).  Like the reference's `infer(&self)` (face_detection.rs:205),
 *     every entry point may be called on one handle from several threads at once: the interpreter state the reference
 *     rebuilds per call (here: activation arena, captured hipGraphs, staging buffers) lives in the handle, so calls on one
 *     handle are serialised by an internal mutex, and a call on a different caller stream than the previous one first waits
 *     on the device for that previous call's work.  Results equal the single-caller ones; for calls that actually overlap
 *     on the GPU use one handle per worker thread / stream.  mi_last_error() is thread-local.
 *   - all outputs are caller-allocated with explicit capacities.
 */
#ifndef MI_FACE_H_
#define MI_FACE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_OK 0
#define MI_EINVAL (-1)   /* bad argument / shape mismatch                                   */
#define MI_EIO (-2)      /* cannot read model file                                          */
#define MI_EMODEL (-3)   /* malformed or unsupported .tflite graph                          */
#define MI_EDEVICE (-4)  /* HIP runtime error, no GPU, or kernels missing for this GPU      */
#define MI_ERANGE (-5)   /* numeric guard of the reference tripped (e.g. letterbox scale)   */
#define MI_ENOMEM (-6)

#define MI_MEM_HOST 0
#define MI_MEM_DEVICE 1

const char *mi_last_error(void);
/* Number of HIP devices visible to the library (0 when none: every create/load then fails with MI_EDEVICE). */
int mi_device_count(void);
const char *mi_version(void);

/* ------------------------------------------------------------------------------------------------------------------
 * Value types crossing the boundary (types.rs)
 * ---------------------------------------------------------------------------------------------------------------- */

/* Detection { data: Array2<f32>[8,2], score: f32 } — types.rs:189-206.
 * data = (xmin,ymin), (xmax,ymax), then 6 keypoints in FaceIndex order (face_detection.rs:91-98), normalised [0,1]. */
typedef struct mi_detection {
    float data[16];
    float score;
} mi_detection;

/* Rect — types.rs:24-36 (rotation in radians, clockwise; normalized = relative to image size). */
typedef struct mi_rect {
    double x_center, y_center, width, height, rotation;
    int normalized;
} mi_rect;

/* Landmark { x, y, z: f64 } — types.rs:176-187. */
typedef struct mi_landmark {
    double x, y, z;
} mi_landmark;

/* FaceDetectionModel — face_detection.rs:117-123. */
enum { MI_FD_FRONT_CAMERA = 0, MI_FD_BACK_CAMERA = 1, MI_FD_SHORT = 2, MI_FD_FULL = 3, MI_FD_FULL_SPARSE = 4 };

#define MI_NUM_FACE_LANDMARKS 468 /* face_landmark.rs:29 */
#define MI_NUM_EYE_LANDMARKS 71   /* iris_landmark.rs:41 */
#define MI_NUM_IRIS_LANDMARKS 5   /* iris_landmark.rs:42 */

/* ------------------------------------------------------------------------------------------------------------------
 * L0 — engine surface: replaces the `tflite` crate as used at face_detection.rs:188,207-257,
 * face_landmark.rs:216,233-290, iris_landmark.rs:150,161-228.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct mi_model mi_model;

/* FlatBufferModel::build_from_file + InterpreterBuilder::build + allocate_tensors (face_detection.rs:188,207-210).
 * Parses the TFL3 flatbuffer, lowers the graph to fused HIP kernels and uploads weights (f16 constants widened to
 * f32 once, instead of the reference's per-call DEQUANTIZE). */
int mi_model_load_file(const char *path, int device, mi_model **out);
int mi_model_load_bytes(const uint8_t *tflite, size_t nbytes, int device, mi_model **out);
void mi_model_free(mi_model *m);

/* get_input_details()[0].dims (face_detection.rs:213-217): dims = {1,H,W,C}. */
int mi_model_input_dims(const mi_model *m, int dims[4]);
/* outputs().len() / tensor_info(outputs()[i]).dims (face_detection.rs:238-249). Returns rank via *rank. */
int mi_model_num_outputs(const mi_model *m);
int mi_model_output_dims(const mi_model *m, int index, int dims[4], int *rank);
size_t mi_model_output_elems(const mi_model *m, int index); /* floats per frame */

/* tensor_data_mut(input).copy_from_slice + invoke + tensor_data(outputs[i]) (face_detection.rs:229-257), batched:
 * in  = f32 NHWC [batch,H,W,C];  outs[i] = f32 [batch, output_elems(i)] in the graph's output order. */
int mi_model_run(mi_model *m, const float *in, int batch, float *const *outs, int mem, void *stream);

/* Copy one intermediate activation (by .tflite tensor index) of the last chunk run, if it was materialised
 * (fused-away tensors return MI_EINVAL).  Debug/test aid; dst is host memory. Returns floats written via *n. */
int mi_model_debug_tensor(mi_model *m, int tensor_index, int frame, float *dst, size_t cap, size_t *n);
/* Human-readable launch plan (one line per kernel launch). Returns bytes needed (incl. NUL). */
size_t mi_model_describe(const mi_model *m, char *buf, size_t cap);
/* Tuning knobs: "chunk" (frames per pass through the net, 0 = whole batch), "graph" (0/1 hipGraph replay),
 * "fuse" (0 = op-by-op kernels, 1 = epilogue fusion, 2 = BlazeBlock fusion, 3 = + frame-resident chains of small-spatial
 * blocks, 4 = + row-pipelined chains of narrow blocks, 5 = + stage programs, operand-layout kernels, fused edges; default 5),
 * "pipe" (blocks per row-pipelined chain, 2..4, 0 = none), "pipe_rows" (0 = automatic: two rows per pipeline step with the 1x1 convs on
 * the 4x4x1 MFMA, one row for odd heights; 1 / 2 = one / two rows per step with packed-FMA 1x1 convs; 4 = one row per step, MFMA),
 * "pipe_band" (rows per band of those chains; 0 = automatic: about one resident set of workgroups over the chip, the best choice for ONE batch in
 * flight; a host that keeps two batches in flight — mi_streams_create_distinct — sets the frame height: fewer pipeline fill steps, and the
 * CUs a short grid leaves idle are the other batch's; BackCamera 256 frames 1.22 -> 1.19 ms per batch),
 * "small_chain" (frames up to which a row-pipelined chain runs one launch per block instead — what keeps a batch of one short;
 * default 16, 0 = never; the stand-alone stride-2 block of that form folds its depthwise bias differently, so one frame's raw
 * outputs differ between a batch <= small_chain and a larger one within the stated 1e-4 tolerance, not bit for bit), "strip" (0 = LDS-ring block kernel for every block),
 * "fork" (0 = output heads run on the trunk's stream instead of beside it), "heads" (side streams the output heads are spread
 * over, 1..4), "mchain" (0 = the 32x32x48 blocks run one launch each instead of one launch per run), "tail" (0 = no stage program takes the several-frames-per-workgroup form of round 5: the round-4 plan),
 * "tail_g" (frames per workgroup of those programs; 0 = chosen per launch from the batch and the LDS a frame needs), "reuse",
 * "lanes"; "band" (the single-launch plan of the single-image entries, below: 0 = never, 1 = the single-image entries only (default), 2 = every run of few
 * enough frames — a tuning / test setting: such a run is synchronised and checked inside the call, and repeated on the batched plan when its launch
 * gave up waiting for its CUs), "band_nw" (workgroups per frame of that plan, 8..256), "band_wide" (0 = its program ends in front of the first stage of
 * more than 128 channels); "stem_fuse" (0 = the face mesh's first convolution keeps a launch of its own instead of running inside the launch of the
 * block pair behind it, from 32 f32 pictures on), "pair_fuse" (0 = two plain BlazeBlocks in a row keep a launch each where one launch has a form for
 * both: the face mesh's 48x48x32 blocks), "mdb_band" (rows per band of those launches, 0 = chosen per launch), "stem_mfma" (the detectors' 5x5 first
 * convolution on f32 tensors, bit-identical results in all three: 1 = on the matrix cores with the window's picture rows kept in registers down a column
 * of 64-pixel tiles (default), 2 = on the matrix cores row-wise, every tile loading the five picture rows of its window, 0 = the packed-FMA kernel;
 * every other value is taken as 1), "stem_run" (output rows per column run of form 1, 1..32; 0 = chosen per launch so that the runs fill the chip, and
 * the row-wise form where that leaves one row per run: a handful of frames), "conv_mfma" (the dense k x k convolutions of f32 graphs with a multiple of
 * 32 input channels, overlapping windows (not k x k stride k) and at most a plain skip — the 3x3 convolutions of a ResNet-style embedding network:
 * 1 = conv_mfma_kernel, an implicit GEMM on the matrix cores (default); 0 = conv_generic_kernel, as before the option existed; each result within the f32
 * bound of its sum — bit-identical in every case measured so far, which is observed and not promised), "conv_bf16" (the same convolutions, whatever
 * "conv_mfma" says, on the bf16 matrix cores, conv_bf16_kernel; tensors stay f32 in memory: 0 = off (default: every bit as without the option); 1 = "bf16":
 * activations and filter values rounded to bf16, round to nearest even, products accumulated in f32 — each result within (K + 4) 2^-24 sum |x w| of the
 * exact convolution of the ROUNDED operands, which are up to 2^-9 relative from the f32 ones; 2 = "bf16x3": every operand split into two bf16 values
 * hi + lo, three products for one (lo w_hi, hi w_lo, hi w_hi) — each result within (3 2^-18 + (3 K + 4) 2^-24) sum |x w| of the exact convolution; an
 * infinite activation gives NaN in this form; values outside 0..2 are clamped; the constants are packed again when it changes), "chain_fixed" (the frame-resident chain launches, chain_kernel: 1 = a launch
 * whose whole form is one of the detectors' — 16x16x96 between its two stride-2 blocks, or 8x8x96, ReLU in every block and a skip connection in every stride-1 block — takes the
 * instantiation with that shape as constants (default); 0 = always the generic kernel; bit-identical results), "chain_sched" (how those fixed-shape
 * instantiations schedule a contraction: 1 = in phases — the LDS reads of the next channel chunk requested first, then the chunk's depthwise FMAs as one
 * block, then its MFMAs as one block (default); 0 = the MFMAs of a chunk interleaved with the next chunk's depthwise taps; bit-identical results).
 * Test hook "test_poison" (0 = off, the default; 1 = 0xFF bytes, a NaN; 2 = 0x7F bytes, 3.39e38): before every run the handle fills its activation
 * arena, its small-batch scratch, its output buffers and, in mi_model_run with host input, its input stage beyond the call's frames — a kernel that
 * reads a byte it did not write first turns up in the results. Weights, programs and the single-launch plan's workspace are never touched.
 * Takes effect on the next run. */
int mi_model_set_option(mi_model *m, const char *key, int value);
/* Reads an option back (same keys), plus the state the engine keeps about the single-launch plan: "band" reads 0 once three single launches in a
 * row have given up (CUs held by other processes, a CU mask) and the handle has stopped using the plan; "band_fail_streak" = such launches in a
 * row so far; "band_wraps" = times the packet workspace was cleared because the 32-bit packet tags were about to wrap (every 2^26 launches). */
int mi_model_get_option(mi_model *m, const char *key, int *value);
/* Host-only: parse + lower a .tflite blob WITHOUT touching a GPU and write the launch plan text (same format as
 * mi_model_describe). Returns bytes needed (incl. NUL), 0 on error (see mi_last_error). Used by CPU-side tests. */
size_t mi_plan_describe(const uint8_t *tflite, size_t nbytes, int fuse_level, char *buf, size_t cap);
/* Measurement aid: runs the plan `reps` times with eager launches and a HIP event between consecutive launches on the
 * handle's stream; writes a JSON array with one record per launch {"kernel","shape","ms","bytes","macs"} (ms = average
 * duration, bytes/macs = algorithmic work of that launch for `batch` frames). in_device = DEVICE pointer.
 * Returns bytes needed (incl. NUL), 0 on error. */
size_t mi_model_profile(mi_model *m, const float *in_device, int batch, int reps, char *buf, size_t cap);
/* Algorithmic traffic of the launch plan per frame (bytes read+written by the kernels as launched, weights
 * included once) and MACs per frame; used by bench.py for the roofline figure. */
int mi_model_plan_stats(const mi_model *m, double *bytes_per_frame, double *macs_per_frame, int *launches);
/* The single-image entries (mi_fd_infer_image ...: one Mat per call, face_detection.rs:205) run a graph that is a first convolution
 * followed by BlazeBlocks / 1x1 convolutions as ONE launch behind that convolution (bandnet_kernels.hip) instead of the batched
 * plan's launches (2x2 stride-2 convolutions and the blocks behind them, whose skip is the 2x2 max of the convolution's input, are stages
 * too: the iris network); a graph that continues with other operators (the face mesh's and the iris network's whole-frame convolutions)
 * runs its leading part that way and the rest on the batched plan's launches.  Returns the workgroups (= CUs held for the launch) such a call of `batch` frames occupies, 0 when the graph has
 * no such form or `batch` is too large for it, negative on error.  Engine option "band" = 0 turns the form off. */
int mi_model_single_launch_workgroups(mi_model *m, int batch);

/* ------------------------------------------------------------------------------------------------------------------
 * L1 — FaceDetection (face_detection.rs:146-362)
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct mi_fd mi_fd;

/* FaceDetection::new(model_type, model_path) — face_detection.rs:153-195. model_dir is a DIRECTORY (NULL = "./models");
 * the file name is chosen by `kind` (face_detection.rs:125-129,163-185). Generates the SSD anchors (366-413). */
int mi_fd_create(int kind, const char *model_dir, int device, mi_fd **out);
/* Same, from bytes already in memory (e.g. after an RCCL broadcast of the frozen .tflite over xGMI). */
int mi_fd_create_from_bytes(int kind, const uint8_t *tflite, size_t nbytes, int device, mi_fd **out);
void mi_fd_free(mi_fd *h);
mi_model *mi_fd_model(mi_fd *h); /* borrowed */
int mi_fd_input_size(const mi_fd *h, int *width, int *height);
int mi_fd_num_anchors(const mi_fd *h);
int mi_fd_anchors(const mi_fd *h, float *out_xy, int cap); /* ssd_generate_anchors, [n][2] */

/* Batched FaceDetection::infer from the tensor stage on (face_detection.rs:222-265): network, decode_boxes,
 * get_sigmoid_score, convert_to_detections, weighted NMS (0.3 / 0.5), detection_letterbox_removal.
 *   in       f32 [batch,H,W,3] in [-1,1] (what image_to_tensor produced)
 *   padding  NULL (no letterbox) or f64 [batch][4] = (left, top, right, bottom) per frame (ImageTensor.padding)
 *   out      [batch][cap_per_frame] detections, descending head-score order; counts[b] = number found in frame b
 *            (may exceed cap_per_frame: only the first cap_per_frame are stored; with MI_MEM_HOST the unused slots are
 *            zeroed, with MI_MEM_DEVICE they are left untouched).  out/counts follow `mem`. */
int mi_fd_infer_tensor(mi_fd *h, const float *in, int batch, const double *padding, mi_detection *out,
                       int cap_per_frame, int *counts, int mem, void *stream);
/* Post-network stage only, on raw outputs (regressors [batch,N,16], classificators [batch,N]). */
int mi_fd_postprocess(mi_fd *h, const float *raw_boxes, const float *raw_scores, int batch, const double *padding,
                      mi_detection *out, int cap_per_frame, int *counts, int mem, void *stream);
/* FaceDetection::infer(&Mat, Option<Rect>) — face_detection.rs:205-267. rgb = 8UC3 RGB rows of `stride` bytes
 * (utils.rs:8-21); roi NULL = whole image. Host pointers. *count = detections found (stored: min(count, cap)). */
int mi_fd_infer_image(mi_fd *h, const uint8_t *rgb, int width, int height, int stride, const mi_rect *roi,
                      mi_detection *out, int cap, int *count);

/* Batched FaceDetection::infer(&Mat, Option<Rect>) — face_detection.rs:205-267 over `batch` equally sized 8UC3 RGB frames
 * (utils.rs:8-21; rows of `stride` bytes, frames `stride*height` bytes apart): image_to_tensor(frame, roi, (w,h),
 * keep_aspect_ratio = true, (-1,1)) with the u8 -> f32 loop of transform.rs:292-301 on the device, the network, decode +
 * sigmoid + weighted NMS, letterbox removal — one call, no f32 frames cross the bus (a 256x256 frame is 196 KB instead
 * of 786 KB).  rois NULL (whole frames) or [batch]; frames / rois / out / counts follow `mem`; out / counts as for
 * mi_fd_infer_tensor. */
int mi_fd_infer_images(mi_fd *h, const uint8_t *frames, int batch, int width, int height, int stride, const mi_rect *rois,
                       mi_detection *out, int cap_per_frame, int *counts, int mem, void *stream);
/* The same for a host feed, split in two so that the copy of one batch overlaps the kernels of the other: submit queues
 * H2D copy (on the slot's own stream), pre-processing, network and post-processing — whose kernel writes detections and counts
 * straight into the slot's pinned, mapped, coherent host block (no result copy is queued) — and returns; collect waits for that
 * slot and hands the results out.  Two slots (0 / 1); a slot must be collected
 * before it is submitted again; `frames` must stay valid until then and should be pinned (mi_host_alloc) — a pageable
 * buffer is copied synchronously by the runtime.  Whole frames (roi = None). */
int mi_fd_submit_images(mi_fd *h, int slot, const uint8_t *frames, int batch, int width, int height, int stride,
                        int cap_per_frame);
int mi_fd_collect(mi_fd *h, int slot, mi_detection *out, int *counts);
/* convert_image_to_mat + FaceDetection::infer(&mat, None) for a STREAM of encoded pictures (utils.rs:8-21 then face_detection.rs:205-267, the
 * first two lines of lib.rs:20-24), two slots.  submit does the serial part of the decoder (markers, Huffman decoding: baseline and progressive)
 * on the calling thread — while the device is still busy with the picture in the other slot — and queues the rest: the coefficients' copy,
 * dequantisation + IDCT + up-sampling + colour conversion (the RGB picture never visits the host), image_to_tensor, the network, the
 * post-processing; collect waits for that slot and returns the detections (and the picture's size; width / height may be NULL).  A slot
 * must be collected before it is submitted again; `bytes` may be released when submit returns.  Results are those of
 * mi_jpeg_decode_rgb + mi_fd_infer_image.  Errors of the stream (MI_EINVAL: not a JPEG of the supported subset) are reported by submit. */
int mi_fd_submit_jpeg(mi_fd *h, int slot, const uint8_t *bytes, size_t nbytes, int cap);
int mi_fd_collect_jpeg(mi_fd *h, int slot, mi_detection *out, int cap, int *count, int *width, int *height);
/* Page-locked host memory for frames handed to mi_fd_submit_images (hipHostMalloc / hipHostFree). */
int mi_host_alloc(size_t bytes, void **out);
void mi_host_free(void *p);

/* ------------------------------------------------------------------------------------------------------------------
 * L1 — FaceLandmark (face_landmark.rs:200-306)
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct mi_fl mi_fl;

/* FaceLandmark::new(model_path) — face_landmark.rs:208-222. model_path is a FILE path (NULL =
 * "./models/face_landmark.tflite"). Fails with MI_EMODEL when the mesh output is narrower than 1404 (244-247). */
int mi_fl_create(const char *model_path, int device, mi_fl **out);
int mi_fl_create_from_bytes(const uint8_t *tflite, size_t nbytes, int device, mi_fl **out);
void mi_fl_free(mi_fl *h);
mi_model *mi_fl_model(mi_fl *h);

/* Batched FaceLandmark::infer from the tensor stage on (face_landmark.rs:252-305): network, face-flag test
 * (sigmoid(flag) <= 0.5 => no landmarks, 292-296), project_landmarks (transform.rs:351-432).
 *   in           f32 [batch,192,192,3] in [0,1]
 *   rois         NULL or [batch] ROI each crop was taken from (Option<Rect>); image_sizes int [batch][2] = (w,h) of the
 *                source image of each ROI (needed when a ROI is not normalised); may be NULL when rois is NULL
 *   landmarks    f32 [batch][468][3] projected landmarks (x,y,z as the reference's f32 values before widening)
 *   present      [batch] 1 when the face flag passed (reference returns an empty Vec otherwise), else 0
 *   raw_flags    optional [batch] raw flag logits (may be NULL) */
int mi_fl_infer_tensor(mi_fl *h, const float *in, int batch, const mi_rect *rois, const int *image_sizes,
                       float *landmarks, int *present, float *raw_flags, int mem, void *stream);
/* FaceLandmark::infer(&Mat, Option<Rect>) over a batch (face_landmark.rs:232-306): frames as the reference's callers hold them
 * (8UC3 RGB, `batch` frames of `height` rows of `stride` bytes, stride*height bytes apart) and one ROI per item — item i reads
 * frame i / items_per_frame (several faces of one frame: items_per_frame > 1).  image_to_tensor(frame, roi, (192,192),
 * keep_aspect_ratio = false, (0,1)) runs on the device (transform.rs:188-309, bit-exact), then the network, the face flag and
 * project_landmarks: no f32 crop crosses the bus (442 KB per ROI through mi_fl_infer_tensor).  rois NULL (whole frames;
 * items_per_frame must be 1) or [batch * items_per_frame]; frames / rois / results follow `mem`; results as mi_fl_infer_tensor
 * with batch * items_per_frame items. */
int mi_fl_infer_images(mi_fl *h, const uint8_t *frames, int batch, int width, int height, int stride, const mi_rect *rois,
                       int items_per_frame, float *landmarks, int *present, float *raw_flags, int mem, void *stream);
/* The same for a continuous host feed, in two halves like mi_fd_submit_images / mi_fd_collect: submit queues the H2D copy of the
 * frames (on the slot's own stream), the warp, the network and the projection — whose kernel writes into the slot's pinned, mapped,
 * coherent host block — and returns; collect waits for that slot and hands the results out (raw_flags may be NULL).  Two slots
 * (0 / 1): the copy of one batch runs beside the kernels of the other.  A slot must be collected before it is submitted again;
 * `frames` must stay valid until then and should be pinned (mi_host_alloc).  Host memory only. */
int mi_fl_submit_images(mi_fl *h, int slot, const uint8_t *frames, int batch, int width, int height, int stride,
                        const mi_rect *rois, int items_per_frame);
int mi_fl_collect(mi_fl *h, int slot, float *landmarks, int *present, float *raw_flags);
/* FaceLandmark::infer(&Mat, Option<Rect>) — face_landmark.rs:232-306. out = 468 landmarks; *count = 0 or 468. */
int mi_fl_infer_image(mi_fl *h, const uint8_t *rgb, int width, int height, int stride, const mi_rect *roi,
                      mi_landmark *out, int cap, int *count);

/* ------------------------------------------------------------------------------------------------------------------
 * L1 — IrisLandmark (iris_landmark.rs:130-248)
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct mi_iris mi_iris;

/* IrisLandmark::new(model_path) — iris_landmark.rs:142-156 (FILE path; NULL = "./models/iris_landmark.tflite").
 * Fails with MI_EMODEL unless the outputs are 213 and 15 wide (172-184). */
int mi_iris_create(const char *model_path, int device, mi_iris **out);
int mi_iris_create_from_bytes(const uint8_t *tflite, size_t nbytes, int device, mi_iris **out);
void mi_iris_free(mi_iris *h);
mi_model *mi_iris_model(mi_iris *h);

/* Batched IrisLandmark::infer from the tensor stage on (iris_landmark.rs:190-246).
 *   in            f32 [batch,64,64,3] in [0,1] (already flipped for right eyes, as image_to_tensor does)
 *   rois/image_sizes as for mi_fl_infer_tensor; padding NULL or f64 [batch][4]; is_right_eye NULL or int [batch]
 *   contour       f32 [batch][71][3], iris f32 [batch][5][3] */
int mi_iris_infer_tensor(mi_iris *h, const float *in, int batch, const mi_rect *rois, const int *image_sizes,
                         const double *padding, const int *is_right_eye, float *contour, float *iris, int mem,
                         void *stream);
/* IrisLandmark::infer(&Mat, Option<Rect>, Option<bool>) over a batch (iris_landmark.rs:158-248): u8 frames + one eye ROI (+
 * is_right_eye) per item, item i reads frame i / items_per_frame (2 = the two eyes of a face).  image_to_tensor(frame, roi,
 * (64,64), keep_aspect_ratio = true, (0,1), flip = is_right_eye) on the device, network, both project_landmarks calls (the
 * letterbox padding of every item stays on the device).  rois NULL (whole frames, items_per_frame 1) or [batch * items_per_frame];
 * is_right_eye NULL (no flips) or int [batch * items_per_frame]; contour f32 [N][71][3], iris f32 [N][5][3]. */
int mi_iris_infer_images(mi_iris *h, const uint8_t *frames, int batch, int width, int height, int stride, const mi_rect *rois,
                         const int *is_right_eye, int items_per_frame, float *contour, float *iris, int mem, void *stream);
/* IrisLandmark::infer(&Mat, Option<Rect>, Option<bool>) — iris_landmark.rs:158-248 -> IrisResults {contour, iris}. */
int mi_iris_infer_image(mi_iris *h, const uint8_t *rgb, int width, int height, int stride, const mi_rect *roi,
                        int is_right_eye, mi_landmark *contour71, mi_landmark *iris5);

/* ------------------------------------------------------------------------------------------------------------------
 * Batched detector -> mesh -> iris pipeline, every stage on the device (BASELINE config 5)
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct mi_pipeline mi_pipeline;

/* Loads the detector selected by `fd_kind` plus face_landmark.tflite and iris_landmark.tflite from `model_dir`
 * (NULL = "./models") — the three handles of the README.md:27-46 / lib.rs:18-40 flow. */
int mi_pipeline_create(int fd_kind, const char *model_dir, int device, mi_pipeline **out);
/* Same, from bytes already in memory (each rank of a multi-GPU job receives the three frozen graphs by RCCL broadcast). */
int mi_pipeline_create_from_bytes(int fd_kind, const uint8_t *fd_tflite, size_t fd_nbytes, const uint8_t *fl_tflite,
                                  size_t fl_nbytes, const uint8_t *iris_tflite, size_t iris_nbytes, int device,
                                  mi_pipeline **out);
void mi_pipeline_free(mi_pipeline *p);
/* The pipeline's three engine handles (borrowed): which = 0 detector, 1 face mesh, 2 iris; NULL otherwise. */
mi_model *mi_pipeline_model(mi_pipeline *p, int which);
/* mi_model_set_option on the three networks of the pipeline (e.g. "lanes": frame ranges on concurrent streams). */
int mi_pipeline_set_option(mi_pipeline *p, const char *key, int value);
/* For each of `batch` equally sized RGB frames (8UC3, rows of `stride` bytes, frames `stride*height` bytes apart):
 *   FaceDetection::infer(frame, None) -> faces[0] -> face_detection_to_roi -> FaceLandmark::infer(frame, roi)
 *   -> iris_roi_from_face_landmarks -> IrisLandmark::infer(frame, left, false) and (frame, right, true)
 * (lib.rs:24-40) without any host round trip between the stages: ROIs, rotated-ROI warps and projections stay on the GPU.
 *   faces        [batch] top-1 detection (zeroed when none)      face_counts [batch] detections found by the detector
 *   landmarks    f32 [batch][468][3]                             present     [batch] 1 = face found and mesh flag passed
 *   eyes         f32 [batch][2][76][3]: left eye then right eye, each 71 eye-contour + 5 iris landmarks (zeros when absent)
 * All pointers follow `mem`. */
int mi_pipeline_run(mi_pipeline *p, const uint8_t *frames, int batch, int width, int height, int stride, mi_detection *faces,
                    int *face_counts, float *landmarks, int *present, float *eyes, int mem, void *stream);
/* The same flow for EVERY face of a frame (a group photo, a two-person call), still without a host round trip: the detector's first
 * `max_faces` (1..16) detections of each frame, in the detector's output order, each through face_detection_to_roi -> FaceLandmark::infer ->
 * iris_roi_from_face_landmarks -> 2 x IrisLandmark::infer exactly as above.  The faces of the batch are compacted on the device into a list of
 * `max_items` (1..32767) ITEMS, in frame order, then detector order: frame b contributes n_b = min(max(face_counts[b], 0), max_faces) faces, and
 * item j = (sum of n_b' for b' < b) + k is face k of frame b while j < max_items.
 *   faces        [batch][max_faces], zeros behind a frame's last detection   face_counts [batch] detections found (may exceed max_faces)
 *   item_frame   [max_items] frame of item j, -1 for an unused slot           item_face   [max_items] k of faces[frame][k], -1 when unused
 *   n_items      [2]: slots used = min(total, max_items); faces (within max_faces) that got no slot = total - slots used
 *   landmarks    f32 [max_items][468][3]   present [max_items]   eyes f32 [max_items][2][76][3]   (zeros in unused slots)
 * `faces` and `face_counts` cover every frame whatever the budget.  COST: the mesh network always runs on max_items items and the iris network on
 * 2 * max_items, whatever the detector finds — launch shapes depend on the arguments alone, so the call reads no count back, stays asynchronous
 * (MI_MEM_DEVICE with a caller's stream: no host synchronisation but the one-off upload when the batch geometry changes) and can be replayed.
 * max_items is part of that geometry, with width and height: calls that alternate between two budgets on one handle upload and synchronise
 * every time, so keep one handle per budget where that matters.
 * Choose max_items for the faces you expect, not batch * max_faces.  This entry always runs the batched plan: it never takes a single-launch
 * plan, so it claims no CUs and has no retry path.  batch <= 2^26.  max_items beyond 32767 is MI_EINVAL before anything is queued (the
 * pre-processing launch has one grid row per item, at most 65535 of them, and the iris stage has 2 * max_items items).  All pointers follow `mem`. */
int mi_pipeline_run_faces(mi_pipeline *p, const uint8_t *frames, int batch, int width, int height, int stride, int max_faces, int max_items,
                          mi_detection *faces, int *face_counts, int *item_frame, int *item_face, int *n_items, float *landmarks,
                          int *present, float *eyes, int mem, void *stream);
/* Host only, no GPU: the item layout the call above produces for these counts (the specification of the device kernel; both go through
 * the same arithmetic).  MI_EINVAL for a null pointer, max_faces outside 1..16, max_items outside 1..2^20 or batch outside 1..2^26. */
int mi_face_items_layout(const int *face_counts, int batch, int max_faces, int max_items, int *item_frame, int *item_face, int *n_items);
/* The same flow from ENCODED pictures, as the reference's own test runs it (lib.rs:18-40: include_bytes!(man.jpg) -> convert_image_to_mat ->
 * FaceDetection::infer -> FaceLandmark::infer -> 2 x IrisLandmark::infer), for a stream of them, two slots (see mi_fd_submit_jpeg): submit decodes the
 * entropy-coded data on the calling thread while the device still works through the other slot's picture, and queues the decoder's sample arithmetic
 * and the three stages; collect waits for that slot.  Outputs as mi_pipeline_run with batch = 1: face = faces[0] (zeros when none), *face_count,
 * landmarks f32 [468][3], *present, eyes f32 [2][76][3]; width / height (may be NULL) = the picture's size.  Host memory. */
int mi_pipeline_submit_jpeg(mi_pipeline *p, int slot, const uint8_t *bytes, size_t nbytes);
int mi_pipeline_collect_jpeg(mi_pipeline *p, int slot, mi_detection *face, int *face_count, float *landmarks, int *present, float *eyes,
                             int *width, int *height);

/* ------------------------------------------------------------------------------------------------------------------
 * mi_tracker — landmark-to-ROI face tracking for `streams` video streams, one face per stream (MediaPipe's num_faces = 1).
 * NOT the reference's behaviour: the reference has no video loop.  This is MediaPipe's: the ROI of frame t+1 comes from the landmarks of
 * frame t, and the detector runs only for a stream that has no face yet or has lost it — composed from the reference's own
 * bbox_from_landmarks (transform.rs:146-165) and bbox_to_roi (transform.rs:44-109), the way iris_roi_from_face_landmarks composes them
 * for the eyes (iris_landmark.rs:268-292).  The per-stream state {ROI, tracked} lives in device memory; a step reads nothing back.
 *
 * TRACKED ROI of landmarks f32 [468][3] (normalised to the frame, as the pipeline writes them): bbox = min / max of x and of y over all 468
 * landmarks (f64); rotation key points = landmarks 33 and 263 (the outer eye corners) in PIXELS, (x * width, y * height);
 * roi = bbox_to_roi(bbox, (width, height), key points, scale (1.5, 1.5), SquareLong).  Valid iff all 936 x / y values are finite, the box
 * is normalised (BBox::normalized), width > 0 and height > 0.
 * DETECT PLAN: the streams with tracked == 0 get the `max_detect` detector slots in cyclic stream order beginning at stream `start`; slot j
 * is the j-th lost stream met from `start` on; det_stream[max_detect] holds -1 in unused slots; n_detect = {slots used, lost streams left
 * without a slot}.  A handle starts at 0 and advances start by max_detect modulo streams after every step, so a stream that stays lost gets
 * a slot at least once in any ceil(streams / max_detect) consecutive steps, however many streams never show a face.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct mi_tracker mi_tracker;

/* Host only, no GPU: the two rules (the specification of the device kernels; both sides go through the same arithmetic).
 * mi_track_roi_from_landmarks: *valid = 0 and a zeroed *roi for an invalid set.  MI_EINVAL for a null pointer or a size below 1.
 * mi_track_detect_layout: tracked [streams], streams 1..2^20, max_detect 1..streams, start 0..streams-1; anything else is MI_EINVAL. */
int mi_track_roi_from_landmarks(const float *landmarks, int width, int height, mi_rect *roi, int *valid);
int mi_track_detect_layout(const int *tracked, int streams, int max_detect, int start, int *det_stream, int *n_detect);

/* A tracker owns its three networks (as mi_pipeline_create / mi_pipeline_create_from_bytes load them) and every buffer it uses: calls on
 * other handles neither see nor pay for it.  streams 1..32767 (the iris stage has 2 * streams items, one per grid row of a launch).
 * Every stream starts lost. */
int mi_tracker_create(int fd_kind, const char *model_dir, int device, int streams, mi_tracker **out);
int mi_tracker_create_from_bytes(int fd_kind, const uint8_t *fd_tflite, size_t fd_nbytes, const uint8_t *fl_tflite, size_t fl_nbytes,
                                 const uint8_t *iris_tflite, size_t iris_nbytes, int device, int streams, mi_tracker **out);
void mi_tracker_free(mi_tracker *t);
/* mi_pipeline_set_option on the tracker's three networks (e.g. "test_poison").  One key is the tracker's own, a measurement aid:
 * "track_launches_only" = 1 makes every later step queue its three own launches (plan, select, update) alone, on what the last full step
 * left in the handle's buffers; tools/track_probe.py times the launches that way.  Such a step is MI_EINVAL, before anything is queued,
 * unless the handle's last full step had the same max_detect, width and height.  Its outputs and the state it leaves mean nothing, so
 * setting the key back to 0 drops the state as mi_tracker_reset(t, -1) does (and synchronises). */
int mi_tracker_set_option(mi_tracker *t, const char *key, int value);
/* One step: `frames` holds `streams` equally sized RGB frames (as mi_pipeline_run's), frame s the next picture of stream s.
 *   1. plan: det_stream / n_detect from the state (one launch)
 *   2. the detector on exactly max_detect (1..streams) items: item j reads frame det_stream[j], an unused slot gets a zero tensor and its
 *      answer is ignored; top-1 detection and its face_detection_to_roi
 *   3. per stream: tracked -> the state's ROI, source 2; else a slot whose detector count is > 0 and whose ROI is valid -> that ROI,
 *      source 1; else source 0
 *   4. face mesh and both eyes of every stream with source != 0, as mi_pipeline_run
 *   5. where present[s] holds and the tracked ROI of its landmarks is valid that ROI becomes the state and tracked = 1; else tracked = 0
 * Outputs (all follow `mem`; streams without a result hold zeros):
 *   faces       [streams] the detection a stream was acquired from (zeros unless source = 1)
 *   face_counts [streams] the detector's count for a stream that held a slot, else 0        source [streams]
 *   rois        [streams] the mi_rect the mesh ran on (zeros for source 0)
 *   landmarks   f32 [streams][468][3]      present [streams]      eyes f32 [streams][2][76][3]
 *   det_stream  [max_detect]               n_detect [2]
 * The first seven lie as mi_pipeline_run's, so mi_render_faces takes them.  COST: the detector always runs on max_detect items, the mesh on
 * `streams` and the iris network on 2 * streams: launch shapes depend on streams and max_detect alone, so with MI_MEM_DEVICE and a
 * caller's stream the step does not synchronise but for the one-off upload when (streams, width, height, max_detect) changes.  Always the
 * batched plan, never a single-launch plan.  A handle's steps are ORDERED: each reads the state the previous one wrote, so steps of one
 * handle on two streams must be ordered by the caller.  MI_EINVAL before anything is queued for a null pointer, max_detect outside
 * 1..streams or a frame geometry the other entries refuse; the state is then untouched.  MI_ERANGE (host memory only, where the counts are
 * read back: a letterbox scale the reference asserts on, as mi_pipeline_run's) is found AFTER the step has run: the outputs are written,
 * the state is the step's and the plan's start has advanced, so the next step goes on from there; mi_tracker_reset starts over. */
int mi_tracker_step(mi_tracker *t, const uint8_t *frames, int width, int height, int stride, int max_detect, mi_detection *faces,
                    int *face_counts, int *source, mi_rect *rois, float *landmarks, int *present, float *eyes, int *det_stream,
                    int *n_detect, int mem, void *stream);
/* Drops the state of stream `stream_index` (it is lost: the detector looks for it again); -1: of every stream, and the plan starts at
 * stream 0 again.  Synchronises. */
int mi_tracker_reset(mi_tracker *t, int stream_index);
/* The state, host memory, synchronising: rois [streams] (zeros for a lost stream), tracked [streams].  set_state writes streams
 * first .. first + n - 1 from rois [n] and tracked [n]. */
int mi_tracker_get_state(mi_tracker *t, mi_rect *rois, int *tracked);
int mi_tracker_set_state(mi_tracker *t, int first, int n, const mi_rect *rois, const int *tracked);

/* ------------------------------------------------------------------------------------------------------------------
 * L1 — FaceEmbeddings (face_embeddings.rs:22-109) with l2_norm / similarity_score (utils.rs:30-50)
 *
 * The MODEL IS THE CALLER'S: the reference does not ship face_embeddings.tflite (its README tells users to download one), so none is
 * shipped here either, the reference's own model could not be fetched, its operators are unknown and it has never been run on this
 * engine.  Any graph made of the operators the engine lowers loads; another operator is refused with the planner's message.  The operators:
 * CONV_2D, DEPTHWISE_CONV_2D, FULLY_CONNECTED (weights_format DEFAULT, constant weights and bias, over a [1,K] tensor or the RESHAPE of a
 * [1,H,W,C] one: it runs as the whole-frame convolution), ADD of two tensors, MUL and ADD by a per-channel or scalar constant (an unfolded batch
 * normalisation: folded into the convolution in front where nothing else reads it, else one launch with the activation behind it), PRELU, RELU,
 * fused RELU / RELU6, MAX_POOL_2D, PAD, RESHAPE, CONCATENATION, RESIZE_BILINEAR, DEPTH_TO_SPACE, DEQUANTIZE / DENSIFY of constants.  That is the
 * operator family of a ResNet-style (ArcFace) float graph; its dense 3x3 convolutions run on the matrix cores (option "conv_mfma").  Pooled heads
 * load as well: AVERAGE_POOL_2D, MEAN over H and W of a [1,H,W,C] tensor (either keep_dims), L2_NORMALIZATION over the last dimension (no fused
 * activation), SUB / DIV by a per-channel or scalar constant (x - c, c - x, x / c; a divisor that is no power of two is a true division), and
 * TRANSPOSE of a rank-4 tensor by a constant perm that keeps the batch axis (the identity is an alias).  ONNX-exported graphs are normalised at
 * load: behind TRANSPOSE (0,3,1,2) the channel-first element-wise operators ([1,C,1,1] / [C,1,1] constants, PAD on axes 2 and 3, MEAN over {2,3},
 * the C,H,W flatten in front of FULLY_CONNECTED) move onto NHWC tensors and the transposes around the convolutions disappear; any other reader
 * gets one transpose launch.  Not lowered: c / x, SUB / DIV / MUL of two tensors, MEAN over other axes, CONCATENATION on the channel axis
 * (Inception-style FaceNet), LOGISTIC and the other activations, quantised graphs.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct mi_fe mi_fe;

#define MI_FE_CHIP_SIZE 112 /* IMG_SIZE, face_embeddings.rs:20 */

/* FaceEmbeddings::new(model_path) — face_embeddings.rs:30-44. model_path is a FILE path (NULL = "./models/face_embeddings.tflite", :36).
 * MI_EINVAL with a message unless the graph maps [1,112,112,3] to ONE output of D >= 1 values per frame ([1,D], as :83-84 reads it, and
 * [1,1,1,D] are both taken); an operator the planner does not lower is MI_EMODEL with the planner's message, which names the operator code. */
int mi_fe_create(const char *model_path, int device, mi_fe **out);
int mi_fe_create_from_bytes(const uint8_t *tflite, size_t nbytes, int device, mi_fe **out);
void mi_fe_free(mi_fe *h);
mi_model *mi_fe_model(mi_fe *h); /* borrowed */
/* D: the doc comment at face_embeddings.rs:29 says 128 or 512; any D >= 1 is taken. */
int mi_fe_features(const mi_fe *h, int *features);

/* Host only, no GPU: the rectangle crop_image_to_bbox cuts for a detection (face_embeddings.rs:101-109 on
 * `faces[k].bbox().scale((width as f64, height as f64))`, types.rs:162-165,219-225) — the specification of the device code; both go
 * through the same arithmetic.  Each of xmin, ymin, xmax, ymax is the detection's f32 widened to f64, times the picture size;
 * rect = {x: xmin as i32, y: ymin as i32, width: (xmax - xmin) as i32, height: (ymax - ymin) as i32}, the differences taken in f64, every
 * cast Rust's `as` (toward zero, saturating, NaN -> 0).  *valid = 0 for a rectangle OpenCV's Mat::roi refuses (0 <= x, 0 <= width,
 * x + width <= cols, likewise for rows: the reference panics on the unwrap at :107) and for width <= 0 or height <= 0. */
int mi_face_chip_rect(const mi_detection *det, int width, int height, int rect[4], int *valid);

/* FaceEmbeddings::infer(&Mat, BBox) — face_embeddings.rs:46-89: bbox = {xmin, ymin, xmax, ymax} in absolute pixels (what the reference's
 * test passes: bbox().scale(size), :128).  crop_image_to_bbox, image_to_tensor(crop, None, (112,112), false, (0,1), false) — the crop is an
 * image of its own: BORDER_CONSTANT 0 applies at the crop's edge, no pixel next to the box is sampled —, the network, l2_norm.
 * rgb = 8UC3 RGB rows of `stride` bytes, host memory; embedding = D floats, host memory.  MI_ERANGE where the reference panics (a
 * rectangle Mat::roi refuses, or an empty one); MI_EINVAL for cap < D. */
int mi_fe_infer_image(mi_fe *h, const uint8_t *rgb, int width, int height, int stride, const double bbox[4], float *embedding, int cap);

/* The same for EVERY item of what mi_pipeline_run_faces left in memory, as it lies there: frames [batch] (8UC3, rows of `stride` bytes,
 * frames stride*height bytes apart), faces [batch][max_faces] (max_faces 1..16), item_frame / item_face [max_items] (max_items 1..32767).
 * Item j is faces[item_frame[j]][item_face[j]]: its rectangle as mi_face_chip_rect, its chip, the network on all max_items chips, l2_norm.
 *   embeddings  f32 [max_items][D]            valid  [max_items]: 1 = the item has an embedding
 *   raw         f32 [max_items][D], may be NULL: the network's output before l2_norm (embeddings[j] == mi_l2_norm(raw[j]) bit for bit)
 *   chips       f32 [max_items][112][112][3], may be NULL: the network's input
 * An item is invalid when its item_frame is -1 (an unused slot), when item_frame / item_face point outside the arrays, or when its rectangle
 * is invalid: valid = 0, its rows of all three outputs are zeros, and neither its frame nor its detection is dereferenced.  A norm of zero
 * gives what the reference gives (IEEE division: NaN).  COST: the network always runs on max_items items — launch shapes depend on the
 * arguments alone, no count is read back, and with MI_MEM_DEVICE and a caller's stream nothing synchronises with the host but the allocation
 * of scratch when max_items grows.  All pointers follow `mem`. */
int mi_fe_infer_face_items(mi_fe *h, const uint8_t *frames, int batch, int width, int height, int stride, const mi_detection *faces,
                           int max_faces, const int *item_frame, const int *item_face, int max_items, float *embeddings, int *valid,
                           float *raw, float *chips, int mem, void *stream);

/* ---- Aligned face chips.  NOT the reference's behaviour: the reference crops the detector's box and resizes it (the two entries above,
 * which keep every bit).  ArcFace-style networks are trained on chips in which the eyes, the nose tip and the mouth corners sit at five fixed
 * positions of the 112 x 112 picture; these entries fit, per face, the least-squares similarity transform (rotation, uniform scale,
 * translation) of the face's points to that template and warp the WHOLE frame by it: the transform is the rotated square ROI
 * {x_center, y_center, side, side, rotation, normalized = 0} and the chip is image_to_tensor(frame, Some(roi), (112,112), false, (0,1), false)
 * (transform.rs:188-234), BORDER_CONSTANT 0 outside the frame.
 * Template (chip pixels), in the order image-left eye, image-right eye, nose tip, image-left mouth corner, image-right mouth corner:
 *   (38.2946, 51.6963) (73.5318, 51.5014) (56.0252, 71.7366) (41.5493, 92.3655) (70.7299, 92.2041)
 * `source` says where an item's points come from; every source ends in n f32 pixel points, which the fit widens to f64:
 *   MI_ALIGN_POINTS     f32 [5][2] pixel coordinates in the template's order, as they are
 *   MI_ALIGN_MESH       the item's 468 mesh landmarks (normalised; x * width, y * height in f64): the eyes are the midpoints of landmarks
 *                       33 / 133 and 362 / 263, the nose tip is landmark 1, the mouth corners are 61 and 291
 *   MI_ALIGN_DETECTION  the detection's key points 0..3 (eyes, nose tip, mouth CENTRE; data[4 + 2i] * width, data[5 + 2i] * height in f64)
 *                       against the four-point template: the first three rows and the mean of the last two
 * The fit (f64, sequential sums, no fused multiply-add; m = mean of the points, mq = mean of the template, d* = the differences to them):
 *   A = sum(dx du + dy dv), B = sum(dx dv - dy du), S = sum(dx dx + dy dy), N = A A + B B, c = A S / N, d = -(B S / N),
 *   side = 112 S / sqrt(N), rotation = atan2(-B, A), centre = m + (c + i d)((56, 56) - mq).
 * It is invalid — and the ROI is then the whole image, {0.5, 0.5, 1, 1, 0, normalized = 1} — when a coordinate is not finite, when S or N is
 * not a positive finite number (all points equal), or when side or the centre is not finite. */
#define MI_ALIGN_POINTS 0
#define MI_ALIGN_MESH 1
#define MI_ALIGN_DETECTION 2

/* Host only: the template of `source` -> xy (the rows behind *n are zeros), *n = 5, or 4 for MI_ALIGN_DETECTION. */
int mi_face_align_template(int source, double xy[5][2], int *n);
/* Host only, no GPU: the fit of n f32 pixel points against the template of `source` — the specification of the device code; both go through
 * the same arithmetic.  n must be the template's n (5; 4 for MI_ALIGN_DETECTION), anything else is MI_EINVAL.  *valid = 0 for an invalid fit. */
int mi_face_align_roi(const float *points_xy, int n, int source, mi_rect *roi, int *valid);
/* Host only: the points of ONE item by the gather rule above — landmarks_or_detection = f32 [468][3] (MI_ALIGN_MESH), a detection's 17 floats
 * (MI_ALIGN_DETECTION) or f32 [5][2] (MI_ALIGN_POINTS: copied) -> points_xy (rows behind *n are zeros), *n. */
int mi_face_align_points(int source, const float *landmarks_or_detection, int width, int height, float points_xy[5][2], int *n);

/* One picture in host memory: the fit of points_xy (n pixel points for the template of `source`, as mi_face_align_roi takes them), the
 * aligned chip of the whole picture (all of it is uploaded), the network, l2_norm.  embedding = D floats, host memory; roi may be NULL.
 * MI_ERANGE for an invalid fit; MI_EINVAL for cap < D or an n that is not the template's. */
int mi_fe_infer_image_aligned(mi_fe *h, const uint8_t *rgb, int width, int height, int stride, const float *points_xy, int n, int source,
                              float *embedding, int cap, mi_rect *roi);

/* The aligned chips of EVERY item of what mi_pipeline_run_faces left in memory, as it lies there.  frames, item_frame, max_items, embeddings,
 * valid, raw, chips, mem and stream are those of mi_fe_infer_face_items; src and gate depend on `source`:
 *   MI_ALIGN_POINTS     src = f32 [max_items][5][2], gate = point_valid [max_items] or NULL
 *   MI_ALIGN_MESH       src = landmarks f32 [max_items][468][3], gate = present [max_items]
 *   MI_ALIGN_DETECTION  src = faces [batch][max_faces] (mi_detection), gate = NULL; item_face [max_items] and max_faces (1..16) are read
 *                       for this source only
 *   rois        mi_rect [max_items], may be NULL: the fitted ROI (the whole-image ROI for an invalid item)
 * An item is invalid when its item_frame is outside 0..batch-1, its gate is 0, its item_face is outside 0..max_faces-1 or its fit is invalid:
 * valid = 0, its rows of embeddings, raw and chips are zeros, and neither its frame nor its points, landmarks or detection is dereferenced.
 * A valid ROI may lie wholly outside the frame: its chip is zeros and it has an embedding.  Two launches in front of the network, as the box
 * path has; launch shapes depend on the arguments alone and nothing is read back.  max_items beyond 32767 is MI_EINVAL before anything is
 * queued.  All pointers follow `mem`. */
int mi_fe_infer_aligned_items(mi_fe *h, const uint8_t *frames, int batch, int width, int height, int stride, int source, const void *src,
                              const int *gate, int max_faces, const int *item_frame, const int *item_face, int max_items, float *embeddings,
                              int *valid, float *raw, float *chips, mi_rect *rois, int mem, void *stream);

/* utils::l2_norm(arr) — utils.rs:30-33: out = in / sqrt(sum in^2), the sum in f32, in index order, the square and the add rounded
 * separately (iter().map().sum::<f32>()).  Host only, bit-identical to the reference's order of operations; out may alias in. */
int mi_l2_norm(const float *in, int n, float *out);
/* utils::similarity_score(a, b) — utils.rs:44-50: dot / (norm_a * norm_b), all three sums f32 and sequential.  Host only. */
int mi_similarity_score(const float *a, const float *b, int n, float *out);
/* out[i][j] = similarity_score(a_i, b_j) for a [n][features] against a gallery b [m][features], on the f32 matrix cores
 * (v_mfma_f32_32x32x2_f32): the norms are the reference's sums bit for bit, the dot products are k-ordered fma chains — within
 * (4 * features + 8) * 2^-24 of the sequential evaluation.  n, m >= 1, features 1..4096; a / b / out follow `mem`.  With MI_MEM_DEVICE and a
 * caller stream the call is asynchronous. */
int mi_similarity_matrix(int device, const float *a, int n, const float *b, int m, int features, float *out, int mem, void *stream);

/* ---- Identification: the k best gallery rows of every query, on the device.
 * The selection rule, stated once (csrc/topk.hpp; this host entry and the kernels go through the same comparator).  For query row i,
 * gallery row j is ELIGIBLE iff S[i][j] > -INFINITY is true: NaN and -inf are never selected — a zero query or a zero gallery row gives NaN
 * through the reference's IEEE division and so matches nobody.  Eligible rows are ordered by score descending under the plain f32 `>`
 * (-0.0 and +0.0 tie), ties by the lower j.  The result is the first k rows of that order; slots beyond the number of eligible rows hold
 * index -1, score -INFINITY (label -1).  The order is total, so the result is exact: no tolerance applies to it.
 * Host only, no GPU: the rule applied to a score matrix scores [n][m]; index [n][k], score [n][k].  k 1..16, n, m >= 1. */
int mi_topk_select(const float *scores, int n, int m, int k, int *index, float *score);

/* A gallery of enrolled embeddings.  rows f32 [m][features] (follows `mem`) are copied ONCE into device memory the handle owns — a
 * host-memory caller does not upload them again on every call; labels int [m] or NULL (the label of a row is its index), HOST memory.
 * The handle also owns the scratch of a call (the partial lists of the kernels' first phase), which has to outlive an asynchronous call.
 * m 1..2^24, features 1..4096 (as mi_similarity_matrix).  MI_EINVAL for a bad argument before anything else; MI_EDEVICE without such a
 * device. */
typedef struct mi_gallery mi_gallery;
int mi_gallery_create(int device, const float *rows, int m, int features, const int *labels, int mem, mi_gallery **out);
void mi_gallery_free(mi_gallery *g);
int mi_gallery_dims(const mi_gallery *g, int *m, int *features);
/* "splits": the column ranges a row of query tiles (128 queries) is spread over, one workgroup each: 0 = automatic (the default: the
 * smallest count with which the launch has a workgroup for every compute unit), otherwise 1..64, clamped to the number of 128-column
 * tiles.  The results do not depend on it.  Any other key is MI_EINVAL. */
int mi_gallery_set_option(mi_gallery *g, const char *key, int value);
int mi_gallery_get_option(mi_gallery *g, const char *key, int *value);
/* queries f32 [n][features]; index / score / label [n][k] (label may be NULL); k 1..16, n >= 1; all pointers follow `mem`.
 * score[i][r] is BIT FOR BIT the value mi_similarity_matrix writes at [i][index[i][r]] for the same operands (both kernels run one tile
 * body), the selection is the rule of mi_topk_select, label[i][r] = labels[index[i][r]], or -1 with index -1.  The [n][m] score matrix
 * never reaches memory: two launches (partial lists per column range, then a merge that writes every one of the n * k slots).
 * The embeddings of mi_fe_infer_face_items ([max_items][D], zeros for invalid items) are a valid `queries` as they lie in device memory:
 * invalid items come out as all -1.
 * Concurrency as the other handles: calls on one gallery are serialised, a call on a different caller stream first waits on the device
 * for the previous one, and with MI_MEM_DEVICE and a caller stream nothing synchronises with the host but the regrowth of scratch when
 * n * splits * k grows.  Argument checks are MI_EINVAL before anything is queued. */
int mi_gallery_topk(mi_gallery *g, const float *queries, int n, int k, int *index, float *score, int *label, int mem, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Host-side helpers the reference exports next to the three structs
 * ---------------------------------------------------------------------------------------------------------------- */
/* transform::bbox_to_roi(bbox, image_size, rotation_keypoints, scale, mode) — transform.rs:44-109.  bbox = {xmin, ymin, xmax,
 * ymax} normalised; rotation_keypoints = {x0, y0, x1, y1} in absolute pixels or NULL; size_mode 0 Default, 1 SquareLong,
 * 2 SquareShort (transform.rs:24-34).  MI_EINVAL when the box is not normalised (the reference's Err). */
int mi_bbox_to_roi(const double bbox[4], int image_w, int image_h, const double *rotation_keypoints, double scale_x,
                   double scale_y, int size_mode, mi_rect *out);
/* transform::bbox_from_landmarks(landmarks) — transform.rs:146-165: {xmin, ymin, xmax, ymax}; MI_EINVAL below 2 landmarks. */
int mi_bbox_from_landmarks(const mi_landmark *landmarks, int count, double bbox_out[4]);
/* face_detection_to_roi(face_detection, image_size, None) — face_landmark.rs:180-198 (SquareLong, scale 1.5). */
int mi_face_detection_to_roi(const mi_detection *det, int image_w, int image_h, mi_rect *out);
/* iris_roi_from_face_landmarks(face_landmarks, image_size) — iris_landmark.rs:268-292 (scale 2.3). */
int mi_iris_roi_from_face_landmarks(const mi_landmark *landmarks468, int image_w, int image_h, mi_rect *left_eye,
                                    mi_rect *right_eye);
/* utils::convert_image_to_mat(im_bytes) — utils.rs:8-21 (cv::imdecode(IMREAD_COLOR) + cvtColor(BGR2RGB)) for JPEG streams:
 * entropy decoding on the host, dequantisation / IDCT / chroma upsampling / colour conversion on the GPU (the arithmetic
 * of libjpeg-turbo's default decoder, bit for bit).  Baseline and extended-sequential Huffman JPEG, 8 bit, grey or YCbCr with
 * h1v1 / h2v1 / h2v2 sampling; progressive (SOF2) streams included; anything else (arithmetic coding, 12-bit, CMYK, other containers) is MI_EINVAL with a message.
 * Also MI_EINVAL, because imdecode gives other pixels than a plain decode would: "RGB-coded JPEG" (libjpeg's rule: no JFIF APP0 and an Adobe APP14
 * with transform 0, or component ids R G B) and "EXIF orientation N" for N = 2..8 (imdecode turns the picture); mi_jpeg_info refuses these too when
 * the segment precedes the frame header.
 * rgb = [height][width][3] u8, at least cap_bytes >= 3*width*height (ask mi_jpeg_info first); follows `mem`. */
int mi_jpeg_info(const uint8_t *bytes, size_t nbytes, int *width, int *height);
int mi_jpeg_decode_rgb(int device, const uint8_t *bytes, size_t nbytes, uint8_t *rgb, size_t cap_bytes, int *width,
                       int *height, int mem, void *stream);
/* update_face_landmarks_with_iris_results(face_landmarks, iris_data_left, iris_data_right) — iris_landmark.rs:380-398:
 * the 71 eye-contour/brow landmarks of each eye replace the face-mesh points they refine (index maps iris_landmark.rs:64-95).
 * out468 may alias face468. */
int mi_update_face_landmarks_with_iris_results(const mi_landmark *face468, const mi_landmark *left_contour71,
                                               const mi_landmark *right_contour71, mi_landmark *out468);
/* transform::image_to_tensor — transform.rs:188-309, on the GPU (rotated-ROI warp, letterbox, resize, flip,
 * normalise).  out = f32 [out_h][out_w][3] (follows `mem`); padding_out[4] = (left, top, right, bottom). */
int mi_image_to_tensor(int device, const uint8_t *rgb, int width, int height, int stride, const mi_rect *roi,
                       int out_w, int out_h, int keep_aspect_ratio, double range_min, double range_max,
                       int flip_horizontal, float *out, double padding_out[4], int mem, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * render.rs — annotations drawn on the device (render.rs:262-479, face_landmark.rs:35-166,324-339,
 * iris_landmark.rs:44-62,312-331; the three imageproc 0.25.0 primitives render_to_image draws through)
 * ---------------------------------------------------------------------------------------------------------------- */

/* Color { r, g, b, a } — render.rs:6-26, as the bytes render_to_image writes (`color.r as u8`, `color.a.unwrap_or(255) as u8`,
 * render.rs:431).  The MI_COLOR_* initialisers are Colors::{BLACK, RED, GREEN, BLUE, PINK, WHITE} (render.rs:28-68) with the
 * alpha render_to_image gives them: `mi_color c = MI_COLOR_RED;`. */
typedef struct mi_color {
    uint8_t r, g, b, a;
} mi_color;
#define MI_COLOR_BLACK {0, 0, 0, 255}
#define MI_COLOR_RED {255, 0, 0, 255}
#define MI_COLOR_GREEN {0, 255, 0, 255}
#define MI_COLOR_BLUE {0, 0, 255, 255}
#define MI_COLOR_PINK {255, 0, 255, 255}
#define MI_COLOR_WHITE {255, 255, 255, 255}

/* AnnotationData variants — render.rs:186-192: doubles per item 2 (x, y), 4 (x_start, y_start, x_end, y_end),
 * 4 (left, top, right, bottom), 4 (the same). */
enum { MI_ANN_POINTS = 0, MI_ANN_LINES = 1, MI_ANN_RECTS = 2, MI_ANN_FILLED_RECTS = 3 };

/* Annotation { data, normalized_positions, thickness, color } — render.rs:207-213.  `data` is `count` items of one kind whose
 * doubles start at index `first` of a frame's coordinate block: first + count * (doubles per item) <= coords_per_frame. */
typedef struct mi_annotation {
    int kind;
    int first, count;
    double thickness;
    mi_color color;
    int normalized;
} mi_annotation;

/* render_to_image(annotations, image, blend_mode) — render.rs:361-479, over `batch` equally sized frames: the same annotation
 * list for every frame, each frame with its own positions (coords [batch][coords_per_frame] f64).
 *   canvas   to_rgba8 of the RGB frame, alpha 255 (render.rs:365).  out_channels 4: `out` is that RGBA picture; 3: alpha is
 *            dropped, and `out` may then BE `frames` (in place) when out_stride == stride; any other overlap of the two is
 *            MI_EINVAL.  Rows of `out` are out_stride bytes, frames out_stride*height bytes apart; the bytes of a row beyond
 *            out_channels*width are never written.
 *   order    annotations in list order, items in list order; a later draw overwrites an earlier one (no blending: blend_mode is
 *            read and never used, render.rs:362), the colour's alpha byte is written as it is.
 *   casts    normalised positions are multiplied by (width, height) in f64 (render.rs:368-406); every cast is Rust's `as`:
 *            truncation toward zero, saturation, NaN -> 0.
 *   points   render.rs:423-433: half = max(thickness as u32 / 2, 1); the filled square of side 2*half at
 *            ((x - half) as i32, (y - half) as i32), x = px as u32 (u32 wrapping subtraction), clipped to the canvas.
 *   lines    render.rs:434-445 + imageproc's BresenhamLineIter on the (as i32 as f32) end points; the thickness is ignored.
 *   rects    render.rs:446-462 (rectangle and "oval" draw the same): Rect::at(left as i32, top as i32).of_size((right - left)
 *            as u32, (bottom - top) as u32), four segments with right = left + w - 1, bottom = top + h - 1.
 *   filled   render.rs:463-473: the same rectangle, filled, clipped to the canvas.  Its colour is the annotation's: a
 *            FilledRectOrOval's own `fill` (render.rs:466) makes a caller split an annotation where the fill changes.
 * Two deviations, because nothing panics or spins across this ABI; both are counted per frame in skipped[batch] (may be NULL):
 *   1. a rectangle whose of_size width or height is 0 (imageproc panics) is not drawn;
 *   2. a line is walked for at most max(width, height) steps, whatever its length: the part of the walk in front of the canvas
 *      is skipped in closed form (integer arithmetic on 2*error), which is exact while every f32 value of the walk is exact.
 *      That holds for |coordinate| <= 2^20 after the i32 cast; a line with an end point beyond that bound — or a hollow
 *      rectangle with an edge beyond it — is not drawn (the reference would walk up to 2^32 steps).
 * anns is HOST memory whatever `mem` says (structure, not data); frames / coords / out / skipped follow `mem`.  The call
 * returns after its work has finished (the annotation list is staged per call). */
int mi_render_annotations(int device, const uint8_t *frames, int batch, int width, int height, int stride,
                          const mi_annotation *anns, int n_anns, const double *coords, long coords_per_frame, uint8_t *out,
                          int out_channels, int out_stride, int *skipped, int mem, void *stream);

/* The arguments of detections_to_render_data (render.rs:262-265), face_landmarks_to_render_data (face_landmark.rs:324-339) and
 * eye_landmarks_to_render_data (iris_landmark.rs:312-331).  draw_* = 0 is the reference's `None` colour (render.rs:272,284) /
 * a group the caller leaves out; bounds and keypoints are also gated by line_width > 0 / point_width > 0 (render.rs:273,285).
 * The thicknesses of the landmark groups are f32 as the reference's Option<f32> (render.rs:317,322). */
typedef struct mi_render_style {
    int draw_bounds;
    mi_color bounds_color;
    int line_width;
    int draw_keypoints;
    mi_color keypoint_color;
    int point_width;
    int draw_mesh;
    mi_color mesh_landmark_color, mesh_connection_color;
    float mesh_thickness;
    int draw_eyes;
    mi_color eye_landmark_color, eye_connection_color;
    float eye_thickness;
} mi_render_style;

/* detections_to_render_data + face_landmarks_to_render_data + 2 x eye_landmarks_to_render_data + render_to_image (lib.rs:42-83)
 * on what mi_pipeline_run / mi_fd_infer_images left in memory; with MI_MEM_DEVICE no coordinate visits the host.  Canvas
 * arguments, drawing rules and skipped[] as mi_render_annotations.  Any of the three groups may be NULL; the annotations are
 * built on the device in this order (all positions normalised, f32 widened to f64 before the multiply as Detection::bbox —
 * types.rs:219-225 — and Landmark do):
 *   faces      [batch][faces_per_frame] + face_counts [batch] (min(count, faces_per_frame) faces, none when negative):
 *              the bounds annotation (hollow rectangles, thickness line_width), then the keypoints annotation: all 8 rows of
 *              `data` of every face, the two box corners included (render.rs:289-299), thickness point_width.
 *   landmarks  f32 [batch][468][3], drawn where present[b] != 0 (present NULL: everywhere): the 124 lines of
 *              FACE_LANDMARK_CONNECTIONS (face_landmark.rs:35-166), then the 468 points.
 *   eyes       f32 [batch][2][76][3], gated like the mesh: for the left eye, then the right eye, the 15 lines of
 *              EYE_LANDMARK_CONNECTIONS (iris_landmark.rs:44-60) over the first 15 contour points, then those 15 points.
 * With MI_MEM_DEVICE and a caller stream the call is asynchronous. */
int mi_render_faces(int device, const uint8_t *frames, int batch, int width, int height, int stride, const mi_detection *faces,
                    const int *face_counts, int faces_per_frame, const float *landmarks, const int *present, const float *eyes,
                    const mi_render_style *style, uint8_t *out, int out_channels, int out_stride, int *skipped, int mem,
                    void *stream);

/* mi_render_style plus the arguments of iris_landmarks_to_render_data (iris_landmark.rs:330-377): draw_iris_oval = 0 / draw_iris_points = 0 are
 * the reference's `None` for oval_color / landmark_color (:331,339,358); iris_thickness is its Option<f64>, 1.0 when None (:335).  `base` is
 * read exactly as mi_render_faces reads its style. */
typedef struct mi_render_items_style {
    mi_render_style base;
    int draw_iris_oval;
    mi_color iris_oval_color;
    int draw_iris_points;
    mi_color iris_landmark_color;
    double iris_thickness;
} mi_render_items_style;

/* The drawing of mi_render_faces for what mi_pipeline_run_faces left in memory: EVERY face of a frame with its mesh, both eyes and both
 * irises — detections_to_render_data, then per face face_landmarks_to_render_data + 2 x eye_landmarks_to_render_data + 2 x
 * iris_landmarks_to_render_data (lib.rs:10,42-83), then render_to_image; with MI_MEM_DEVICE no coordinate and no count visits the host.
 * Canvas arguments, out_channels 3 or 4, the in-place rule (out may BE frames with out_channels 3 and out_stride == stride; any other overlap
 * is MI_EINVAL), the drawing rules, skipped[batch] (may be NULL) and the two deviations counted in it (a rectangle whose of_size width or
 * height is 0 is not drawn; a line's walk is bounded by the canvas and a line or hollow rectangle with |coordinate| > 2^20 after the i32 cast
 * is not drawn) are those of mi_render_annotations.
 *   faces       [batch][max_faces] + face_counts [batch], max_faces 1..16: exactly as faces / face_counts / faces_per_frame of mi_render_faces.
 *               The three may be NULL / NULL / anything together.
 *   item_frame  [max_items] and n_items as mi_pipeline_run_faces / mi_face_items_layout write them (max_items 1..32767); only n_items[0] is
 *               read.  The used slots are the first clamp(n_items[0], 0, max_items), their frame indices non-decreasing.  Frame b draws the
 *               contiguous run of slots [lower_bound(b), lower_bound(b + 1)) of that prefix (the halving search for the first slot whose frame
 *               is not below its argument), in ascending slot order.  item_frame values are only ever compared, never used as an address: a
 *               list that breaks the ordering draws some subset of its items (a slot inside a frame's run is drawn only where its frame IS
 *               that frame) and never reads or writes outside the arrays' stated sizes.
 *   landmarks   f32 [max_items][468][3], eyes f32 [max_items][2][76][3] (71 contour rows, then the 5 iris rows: Center, Left, Top, Right,
 *               Bottom — IrisIndex), present [max_items]: item j is drawn only where present[j] != 0; present NULL: every used slot.
 *               landmarks and eyes may each be NULL; either of them without item_frame and n_items is MI_EINVAL.
 * The annotation list of frame b, in this order (all positions normalised, f32 widened to f64 before the multiply, every cast Rust's `as`):
 *   1. the bounds annotation, then the keypoints annotation of the frame's faces, as mi_render_faces;
 *   2. for each item of the frame, in slot order, each group gated by its draw_* flag: mesh lines, mesh points; left-eye lines, points;
 *      right-eye lines, points; left iris oval, left iris points; right iris oval, right iris points.
 *   iris oval   iris_landmark.rs:339-356 with get_iris_diameter (:401-418), in f64, W = width, H = height:
 *               d(a, b) = sqrt((ax*W - bx*W)^2 + (ay*H - by*H)^2); radius = (d(Top, Bottom) + d(Left, Right)) / 2 / 2; radius_h = radius / W,
 *               radius_v = radius / H; one RectOrOval(cx - radius_h, cy - radius_v, cx + radius_h, cy + radius_v), normalised, thickness
 *               iris_thickness, drawn as render_to_image draws an oval: the hollow rectangle (render.rs:446-462).  The divide by W and the
 *               later multiply by W are both done, as in the reference (two roundings).  draw_iris_oval with width < 2 or height < 2 is
 *               MI_EINVAL (the reference's Err, :342-344).
 *   iris points the five iris landmarks as one points annotation (:358-369), thickness iris_thickness: half = max(thickness as u32 / 2, 1).
 * With MI_MEM_DEVICE and a caller stream the call is asynchronous; MI_MEM_HOST stages its operands as mi_render_faces does. */
int mi_render_face_items(int device, const uint8_t *frames, int batch, int width, int height, int stride, const mi_detection *faces,
                         const int *face_counts, int max_faces, const int *item_frame, const int *n_items, int max_items,
                         const float *landmarks, const int *present, const float *eyes, const mi_render_items_style *style, uint8_t *out,
                         int out_channels, int out_stride, int *skipped, int mem, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Multi-GPU: the one exchange of the sharded path — the frozen .tflite bytes go once from `root` to
 * every rank over RCCL (ncclBroadcast, ncclUint8, xGMI inside a node); every rank then builds its handles with
 * mi_*_create_from_bytes (the counterpart of FlatBufferModel::build_from_file, face_detection.rs:188, on ranks that have no
 * file).  One process per GPU; no PyTorch needed (librccl is loaded at call time).  Rendezvous: `root` writes the ncclUniqueId
 * to `id_path` (a file every rank of the node can read, e.g. under /dev/shm; a fresh name per broadcast), the other ranks wait
 * up to timeout_ms (< 0: for ever) for it.  The root removes whatever an earlier run left under that name before it publishes, and the file
 * carries the job's shape (world, root): a file of another shape is never accepted; a stale file of the same shape is caught by the bound on the
 * communicator set-up — with timeout_ms >= 0 ncclCommInitRank runs under max(timeout_ms, 10 s) and the call fails with MI_EIO instead of
 * hanging.  buf: HOST memory of nbytes on every rank — the data on `root`, the receive
 * buffer elsewhere.  device: this rank's GPU ordinal.  Collective: every rank of `world` must call it. */
int mi_dist_broadcast_bytes(const char *id_path, int rank, int world, int root, int device, uint8_t *buf, size_t nbytes,
                            int timeout_ms);

/* ------------------------------------------------------------------------------------------------------------------
 * Two batches in flight.  Every batched entry takes a stream; a host that alternates consecutive batches between two handles
 * on two streams lets the tail of batch n run beside the head of batch n + 1 (BackCamera 256 frames 1.26 -> 1.22 ms per
 * batch, face mesh 512 ROIs 0.93 -> 0.81 ms, detector -> mesh -> iris on 128 frames 2.70 -> 2.14 ms).
 * The two streams must not share a hardware queue — HIP hands its few queues (GPU_MAX_HW_QUEUES, 4 by default) out to
 * streams in the order they are first used, work on two streams of one queue runs strictly in order, and no HIP call tells
 * which queue a stream has.  mi_streams_create_distinct creates n (1 .. 4) hipStream_t's (hipStreamNonBlocking) that were
 * TESTED to run side by side (an idle wave of 40 us on all of them at once) and stores them in streams[0 .. n-1];
 * MI_EDEVICE when it cannot find that many.  The handles' own side streams sit on the same queues, so which of the distinct
 * queues is the best partner still differs by tens of percent: a host that cares times a few batches per candidate, as
 * bench.py does.  mi_streams_destroy synchronises and destroys them.  No counterpart in the reference (CPU only). */
int mi_streams_create_distinct(int device, int n, void **streams);
int mi_streams_destroy(int device, int n, void **streams);

#ifdef __cplusplus
}
#endif
#endif /* MI_FACE_H_ */
