/*
 * ssp.h — C-ABI of libsspgpu.so: the MI355X (gfx950) drop-in for the MFCC -> GMM-UBM /
 * d-vector scoring hot path of kleinzcy/speech_signal_processing.
 *
 * The reference is pure Python and has no FFI for this path; each entry
 * point below names the reference code it replaces.  Host code (Python, ctypes) keeps the
 * reference's call surface and dispatches here.  Plain pointers and sizes only.
 *
 * Conventions
 *   - every function returns SSP_OK (0) or a negative ssp_status; ssp_last_error() returns a
 *     thread-local message for the last failure on the calling thread.  Nothing aborts.
 *   - `where` = SSP_HOST (0): bulk arrays are host pointers, the library stages them through
 *     device scratch the ctx keeps between calls (up to 8 buffers of at most 64 MiB; larger
 *     operands get a buffer of their own for the call — except the batches of ssp_mfcc_run(_i16),
 *     ssp_gmm_score (precision 0 / 2) and ssp_cosine_identify(2) (precision 0, arg-min / minimum)
 *     above two slices (SSP_HOST_SLICE_MB, 64 MiB): those go through a ring of three slice-sized
 *     slots, copied in ahead of the kernels that consume them);  SSP_DEVICE (1): bulk arrays are
 *     device pointers on the ctx's device.
 *   - alignment: a device array needs only the natural alignment of its element type (4 bytes
 *     for float / int32, 2 for int16, 1 for uint8) — a slice `big[1:1 + n]` of a larger array is
 *     a valid argument, and an int16 batch may start on an odd sample.  16-byte alignment is a
 *     matter of speed only: several kernels move 16 bytes per lane from or to an aligned base and
 *     fall back to element-wise moves otherwise (ssp_gru_forward writes an aligned seq_out in
 *     place and copies any other out of its workspace), with bit-identical results.  No entry
 *     point refuses an alignment (tests/test_gpu_alignment.py).  Host arrays are only ever read
 *     and written with memcpy.
 *   - segment offsets (per-utterance sample / frame offsets) are small host-side metadata:
 *     they are always HOST int64 arrays and are uploaded once into an ssp_segments handle.
 *   - one ssp_ctx = one HIP device + one stream.  A ctx is not thread-safe; distinct ctxs are.
 *   - all kernels are asynchronous on the ctx stream; SSP_HOST calls and calls that return
 *     kernel_ms synchronise before returning.  kernel_ms (nullable) receives the device time
 *     of the call's kernels measured with hipEvents on the ctx stream.
 */
#ifndef SSP_H_
#define SSP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSP_ABI_VERSION 4 /* 4: ssp_mfcc_run_i16, sliced host-fed ssp_mfcc_run, ssp_calibrate, precision = auto (ssp_gmm_score 4, ssp_cosine_identify2 3); 3: ssp_cosine_identify2 (precision), ssp_mfcc_plan_set_flags; 2: ssp_comm_* / ssp_allgather / ssp_allreduce_sum; ssp_gmm_score precision = 1 re-scores close calls in fp32 (host sync) */

typedef enum {
    SSP_OK = 0,
    SSP_ERR_INVALID = -1,     /* bad argument / shape */
    SSP_ERR_UNSUPPORTED = -2, /* valid request the kernels do not cover */
    SSP_ERR_HIP = -3,         /* HIP runtime error (message has hipGetErrorString) */
    SSP_ERR_NOMEM = -4,
    SSP_ERR_NODEVICE = -5
} ssp_status;

enum { SSP_HOST = 0, SSP_DEVICE = 1 };

typedef struct ssp_ctx ssp_ctx;
typedef struct ssp_segments ssp_segments;
typedef struct ssp_mfcc_plan ssp_mfcc_plan;
typedef struct ssp_gmm ssp_gmm;
typedef struct ssp_gmm_map ssp_gmm_map;
typedef struct ssp_gmm_full ssp_gmm_full; /* full-covariance GMMs packed for the MFMA scorer */
typedef struct ssp_ivector ssp_ivector;   /* a UBM and a total-variability matrix packed for i-vector extraction and the E-step */
typedef struct ssp_plda ssp_plda;         /* enrolled speakers of a diagonalised PLDA model packed for the MFMA log-likelihood-ratio sweep */
typedef struct ssp_dnn ssp_dnn;           /* a fully connected network packed for the MFMA forward pass */
typedef struct ssp_lstm ssp_lstm;         /* one LSTM layer packed for the recurrent MFMA forward pass */
typedef struct ssp_gru ssp_gru;           /* one GRU layer packed for the per-step MFMA forward pass */
typedef struct ssp_xvector ssp_xvector; /* an x-vector network (frame layers, pooling, segment layers) with its workspace */
typedef struct ssp_dnn_trainer ssp_dnn_trainer; /* a fully connected network with its gradients and Adam state, for training */

/* MFCC dialect knobs.  Three presets are built by the host side:
 *   in-repo  utils/processing.py:19-144  (Hamming, |X|/L, 40 talkbox filters folded, log10(.+1e-8), c0..c12)
 *   sidekit  sidekit.frontend.features.mfcc as called at GMM_UBM.py:89 / d_vector.py:91
 *   librosa  librosa.feature.mfcc as called at MFCC_DTW.py:28-31 */
typedef struct {
    int32_t sample_rate;
    int32_t win_len;      /* samples per analysis window (<= n_fft) */
    int32_t hop;
    int32_t n_fft;        /* power of two, 64..4096 */
    int32_t n_filt;       /* rows of the filterbank table */
    int32_t n_ceps;       /* rows of the DCT table */
    int32_t frame_mode;   /* 0 floor, no pad (sidekit) | 1 ceil, zero-pad tail (utils/processing.py:27) | 2 centred, reflect (librosa) */
    int32_t preemph_mode; /* 0 none | 1 per frame: y[0]=x[0]-a*x[0], y[n]=x[n]-a*x[n-1] */
    float preemph;
    int32_t spec_power;   /* 1 |X| | 2 |X|^2 */
    float spec_scale;     /* multiplies the magnitude / power (1/L for the in-repo dialect, utils/processing.py:139) */
    int32_t log_mode;     /* 0 ln | 1 log10 | 2 10*log10 */
    int32_t floor_mode;   /* 0 none | 1 log(x+eps) (utils/processing.py:105) | 2 log(max(eps,x)) (librosa power_to_db) */
    float eps;
    float top_db;         /* <0 off; else clamp log-mel to (utterance max - top_db) (librosa power_to_db) */
    int32_t delta_order;  /* 0 | 1 [c,dc] (GMM_UBM.py:90-91) | 2 [c,dc,ddc] */
    int32_t delta_N;      /* regression half-width (GMM_UBM.py:53: N=2) */
    int32_t cmvn;         /* 1: per-utterance sklearn.preprocessing.scale (GMM_UBM.py:93) */
} ssp_mfcc_cfg;

int ssp_abi_version(void);
const char* ssp_last_error(void);

/* ---- context: device + stream ------------------------------------------------------- */
/* borrow_stream != 0: `stream` is the caller's hipStream_t (e.g. torch's current stream; NULL = the HIP default
 * stream) and all work is enqueued on it;  borrow_stream == 0: the library creates and owns a stream. */
int ssp_ctx_create(int device, void* stream, int borrow_stream, ssp_ctx** out);
int ssp_ctx_destroy(ssp_ctx* ctx);
/* test aid: fill the LDS of every CU with one 32-bit pattern (e.g. a NaN), so that a kernel reading LDS it never wrote shows up
 * deterministically in the parity tests instead of depending on what the previous kernel left behind */
int ssp_debug_poison_lds(ssp_ctx* ctx, uint32_t pattern);
int ssp_ctx_sync(ssp_ctx* ctx);
/* measurement aid (bench.py `env.calibration`): what this box sustains on two textbook loads, each run for about target_ms
 * milliseconds (<= 0: 20) on the ctx stream and timed with HIP events — a float4 copy of 1 GiB buffers (GB/s, read + write) and
 * eight packed-fp32 FMA chains per lane on every SIMD (TFLOP/s).  Blocks until both are measured; copy_ms / fma_ms may be NULL. */
int ssp_calibrate(ssp_ctx* ctx, double target_ms, double* copy_gbs, double* fma_tflops, double* copy_ms, double* fma_ms);
/* ordering against another stream of the same device without a host wait (a ctx that owns its stream, called with device pointers
 * produced / consumed on the caller's stream): wait = the ctx stream waits for everything queued on other_stream so far;
 * signal = other_stream waits for everything queued on the ctx stream so far.  other_stream: hipStream_t (NULL = the default stream) */
int ssp_ctx_wait_stream(ssp_ctx* ctx, void* other_stream);
int ssp_ctx_signal_stream(ssp_ctx* ctx, void* other_stream);

/* ---- collectives (multi-GPU: one process and one ctx per GPU) ----------
 * Utterances shard across ranks with no data-path collective (GMM_UBM.py:183-197 and d_vector.py:315-318 have no cross-utterance
 * term); models / centroids are replicated.  The one exchange step is the all-gather of the per-utterance decision records after
 * scoring — (int32 argmax, float best, float ubm) = 12 bytes per utterance.  RCCL (rings over xGMI inside a node) is loaded at
 * run time the first time a communicator is asked for; a ctx without a communicator is a world of one.
 *   rank 0: ssp_comm_unique_id(id) -> ship the 128 bytes to every rank (file, socket, MPI, torch store: the caller's transport)
 *   every rank: ssp_comm_init(ctx, rank, nranks, id)    (blocks until all ranks have called it)
 *   ssp_allgather(ctx, send, recv, bytes): DEVICE pointers; recv holds nranks * bytes, rank r's block at r * bytes; asynchronous on
 *   the ctx stream (ssp_ctx_sync before the host reads recv).  Ragged shards: gather the counts first, then padded blocks.
 *   ssp_allreduce_sum(ctx, buf, count, is_f64): in-place sum of float / double DEVICE arrays (centroid sums d_vector.py:310-313,
 *   EM sufficient statistics over utterance shards). */
#define SSP_COMM_ID_BYTES 128
int ssp_comm_unique_id(void* id_out /* HOST byte[128] */);
int ssp_comm_init(ssp_ctx* ctx, int rank, int nranks, const void* unique_id /* HOST byte[128] */);
int ssp_comm_destroy(ssp_ctx* ctx); /* (also done by ssp_ctx_destroy) */
int ssp_comm_info(const ssp_ctx* ctx, int* rank, int* nranks);
int ssp_allgather(ssp_ctx* ctx, const void* send, void* recv, size_t bytes_per_rank);
int ssp_allreduce_sum(ssp_ctx* ctx, void* buf, size_t count, int is_f64);

/* ---- segments: per-utterance offsets (host metadata -> device-resident) ------------- */
/* offsets: HOST int64[n_seg+1], non-decreasing, offsets[0] >= 0. */
int ssp_segments_create(ssp_ctx* ctx, const int64_t* offsets, int64_t n_seg, ssp_segments** out);
int ssp_segments_destroy(ssp_segments* seg);
int ssp_segments_count(const ssp_segments* seg, int64_t* n_seg, int64_t* total);
int ssp_segments_read(const ssp_segments* seg, int64_t* offsets_out /* HOST int64[n_seg+1] */);

/* ---- MFCC: replaces utils.processing.MFCC (utils/processing.py:110-144), sidekit mfcc call
 *      sites (GMM_UBM.py:89, d_vector.py:91), librosa call site (MFCC_DTW.py:29), the delta
 *      loop (GMM_UBM.py:53-69) and preprocessing.scale (GMM_UBM.py:93) as ONE fused pass ---- */
/* window: HOST float[win_len]; fbank: HOST float[n_filt x (n_fft/2+1)] row-major (already folded
 * for the in-repo dialect); dct: HOST float[n_ceps x n_filt] row-major. */
int ssp_mfcc_plan_create(ssp_ctx* ctx, const ssp_mfcc_cfg* cfg, const float* window, const float* fbank,
                         const float* dct, ssp_mfcc_plan** out);
int ssp_mfcc_plan_destroy(ssp_mfcc_plan* plan);
/* SSP_MFCC_REPRODUCIBLE: the float32 bits of an utterance's features do not depend on the batch it is in, its place in it, or the
 * machine's CU count.  By default small batches cut utterances into short chunks for latency (each agrees with the uncut utterance to
 * rounding in the delta-delta block) and machine-filling batches scale inside the kernel (cmvn; rounding again): with the flag every
 * cut chunk recomputes 16 frames of history, which reproduces the uncut bits, scaling always runs as the stand-alone kernel and the
 * 2048-point dialects always take the second-pass clamp + DCT.  Costs latency on single-utterance calls (about 30 % more frames per
 * chunk) and about 15 % on machine-filling batches with cmvn.  (Holds for finite features: a step whose window holds a non-finite
 * cepstrum takes a term-by-term path whose finite rows agree with the matrix-core path to rounding.) */
#define SSP_MFCC_REPRODUCIBLE 1u
int ssp_mfcc_plan_set_flags(ssp_mfcc_plan* plan, uint32_t flags);
int ssp_mfcc_num_frames(const ssp_mfcc_cfg* cfg, int64_t n_samples, int64_t* n_frames);
int ssp_mfcc_out_dim(const ssp_mfcc_cfg* cfg, int32_t* d_out);
/* frame segments derived from sample segments with the plan's framing rule */
int ssp_mfcc_frame_segments(ssp_mfcc_plan* plan, const ssp_segments* sample_seg, ssp_segments** frame_seg_out);
/* samples: float[total samples]; feats_out: float[total frames x d_out] row-major.
 * variant: 0 auto | 1 generic kernel (any cfg) | 2 fused n_fft == 512 kernel, one workgroup per utterance chunk | 3 n_fft == 512 wave-stream
 * kernel (every wave walks its own chunk; DCT / delta / delta-delta on the matrix cores; 13 cepstra, <= 40 filters, N = 2 deltas: the
 * sidekit call sites with or without scaling and the in-repo MFCC; a dense-band instance for the PLP front end; utterances may start at
 * any sample) | 4 n_fft == 2048 wave-stream kernel (no deltas: MFCC_DTW.py:28-31's librosa dialect and frameSize 2048; log filterbank rows
 * and utterance maxima, then the clamp + DCT in the same wave for single-chunk utterances or as a second pass).  An explicit 2 / 3 / 4
 * answers SSP_ERR_UNSUPPORTED when the cfg is not covered; auto picks 3, then 2 (n_fft == 512), 4 (n_fft == 2048), then 1. */
int ssp_mfcc_run(ssp_mfcc_plan* plan, const ssp_segments* sample_seg, const ssp_segments* frame_seg,
                 const float* samples, float* feats_out, int where, int variant, float* kernel_ms);
/* Host-fed batches (where = SSP_HOST — what the reference-shaped callers hand over: GMM_UBM.py:24-50 reads the wav files into host
 * arrays, :86-93 loops over them).  Up to two slices (SSP_HOST_SLICE_MB, default 64 MiB of fp32 samples) a batch is staged whole; larger
 * ones run as a pipeline over runs of whole utterances: slice i + 1 copies in while slice i computes and slice i - 1's features copy
 * back (three streams, a ring of three slots kept on the ctx).  Pinned host memory (hipHostMalloc / torch pin_memory) makes the copies
 * asynchronous and full rate; pageable memory works at the runtime's staging rate.  kernel_ms then spans the pipeline on the ctx stream.
 *
 * ssp_mfcc_run_i16: the same pass on int16 PCM — what utils.tools.read (utils/tools.py:45-47, scipy.io.wavfile) returns and the
 * reference's extractors receive (GMM_UBM.py:86-93, d_vector.py:80-98).  Samples are taken at their integer value (no 1/32768: sidekit's
 * mfcc computes on the integers as they are); half the bytes cross PCIe and a widening kernel on the device feeds the same MFCC
 * kernels (bit-identical to ssp_mfcc_run on the float32 of the same integers).  where = SSP_DEVICE: int16 device array, widened
 * slice by slice through the same ring. */
int ssp_mfcc_run_i16(ssp_mfcc_plan* plan, const ssp_segments* sample_seg, const ssp_segments* frame_seg,
                     const int16_t* samples, float* feats_out, int where, int variant, float* kernel_ms);
/* ssp_mfcc_run_list: the same pass on a LIST of host arrays, one per utterance, as the reference's callers hold them
 * (GMM_UBM.py:72-118 extract_feature, d_vector.py:80-98), without first concatenating them on the host.  utt: HOST array of n pointers
 * (n = sample_seg's count); utterance u is sample_seg's length u of sample_type 0 float32 | 1 int16, read straight from the caller's
 * (pageable or pinned) arrays; a null pointer only for a zero-length utterance.  feats_out: HOST, contiguous (total frames x d_out) of
 * out_type 0 float32 | 1 float64 (widened exactly).  sample_seg must start at sample 0 and frame_seg at frame 0.  Same kernels, same
 * slicing and one-piece / ring decisions as ssp_mfcc_run / ssp_mfcc_run_i16 on the concatenation of the list: bit-identical features.
 * Worker threads (SSP_HOST_THREADS, default min(8, hardware threads), at most 16; they make no HIP call) gather the utterances into
 * pinned slots kept on the ctx — slice i + 1 while slice i copies and computes — and copy or widen the features out of pinned slots.
 * A bad argument answers SSP_ERR_INVALID before any GPU work. */
int ssp_mfcc_run_list(ssp_mfcc_plan* plan, const ssp_segments* sample_seg, const ssp_segments* frame_seg, const void* const* utt,
                      int sample_type, void* feats_out, int out_type, int variant, float* kernel_ms);

/* ---- stand-alone framing and cepstrum steps of the in-repo dialect (kept for API parity; ssp_mfcc_run fuses them) ---- */
/* utils.processing.enframe (utils/processing.py:19-38): frame i = x[i*step : i*step+frame_size], zero padded tail, times
 * window; n_frames = ceil(n/step).  frames_out: float[frame_size x n_frames] row-major, exactly the reference's
 * ndarray (element (k, i) = windowed sample k of frame i). */
int ssp_enframe(ssp_ctx* ctx, const float* samples, int64_t n, int32_t frame_size, int32_t step, const float* window /* HOST float[frame_size] */,
                float* frames_out, int where, float* kernel_ms);
/* utils.processing.stMFCC (utils/processing.py:91-107) on a batch of spectra: out = DCT(log(X . fbank^T (+eps | floor)))
 * X: float[n_rows x n_bins]; fbank: HOST float[n_filt x n_bins]; dct: HOST float[n_ceps x n_filt]; out: float[n_rows x n_ceps].
 * log_mode / floor_mode / eps as in ssp_mfcc_cfg. */
int ssp_cepstrum(ssp_ctx* ctx, const float* X, int64_t n_rows, int32_t n_bins, const float* fbank, int32_t n_filt,
                 const float* dct, int32_t n_ceps, int32_t log_mode, int32_t floor_mode, float eps, float* out, int where,
                 float* kernel_ms);

/* magnitude (power = 1) or power (2) spectrum, scaled, from rows of [re(0..n_bins) | im(0..n_bins)] — the |FFT|/L of
 * utils/processing.py:137-139 when the transform itself ran as a DFT-matrix product (ssp_dense_forward) for frame sizes
 * that are not powers of two.  reim: float[n_rows x 2 n_bins]; out: float[n_rows x n_bins]. */
int ssp_spectrum_abs(ssp_ctx* ctx, const float* reim, int64_t n_rows, int32_t n_bins, float scale, int32_t power, float* out,
                     int where, float* kernel_ms);

/* ---- stand-alone delta / CMVN on feature matrices (GMM_UBM.delta, preprocessing.scale) - */
int ssp_delta(ssp_ctx* ctx, const float* feats, const ssp_segments* frame_seg, int32_t dim, int32_t N,
              float* out, int where, float* kernel_ms);
int ssp_cmvn(ssp_ctx* ctx, const float* feats, const ssp_segments* frame_seg, int32_t dim,
             float* out, int where, float* kernel_ms);

/* ---- sliding-window normalisation, feature warping and speech-frame selection (featnorm.hip).  An extension: the reference scales once
 * per utterance (ssp_cmvn), which suits its 3 s clips; long recordings and sessions whose channel drifts are normalised over a window of
 * about 3 s, and the non-speech frames are dropped before any statistics are taken.  The counterparts — Kaldi's apply-cmvn-sliding
 * (center=true), sidekit's cep_sliding_norm and stg, the feature warping of Pelecanos and Sridharan — are recalled, parity unpinned:
 * none of them is at hand and the reference has no such step.  The float64 restatement in tests/featnorm_oracle.py is the yardstick.
 *
 * The window of frame t of an utterance of T frames is centred and slid back inside the utterance: lo = t - window / 2 (integer
 * division), hi = lo + window; if lo < 0: hi -= lo, lo = 0; if hi > T: lo -= hi - T, hi = T, lo = max(lo, 0).  Every window holds
 * min(window, T) frames and contains t.  Columns are independent.  NaN entries (the silent frames of a dialect without a log floor) are
 * left out of the window's statistics and ranks and come out as NaN; n below is the number of non-NaN entries of the column in the window.
 *   mode 0: y = x - mean over the n entries;  mode 1: y = (x - mean) / deviation about that mean (ddof 0; a deviation below
 *   10 * 2^-23 becomes 1, ssp_cmvn's rule).  A +-inf inside a window gives the non-finite result float64 arithmetic gives on that
 *   window alone, and never reaches a frame whose window does not hold it.  The error does not grow with T.
 *   mode 2 (feature warping): k = 2 #{x_s < x_t} + #{x_s == x_t} over the n entries (the frame itself included, so 1 <= k <= 2n - 1),
 *   y = phi^-1(k / 2n): (rank - 1/2) / n without ties, the mid-rank with ties; +-inf rank like any value.  The count is exact and
 *   phi^-1 comes from the table of ssp_featnorm_table: the device adds no error of its own.
 * feats, out: float[frames x dim] laid out by frame_seg, which need not start at row 0 (rows in front of it are neither read nor
 * written); 1 <= window <= 1024, 1 <= dim <= 4096, utterances of any length, empty ones anywhere.  out == feats is SSP_ERR_INVALID
 * and arrays that overlap in any other way are not supported: tiles read their neighbours' rows.  Device pointers at any 4-byte
 * alignment; the device path returns without a host wait (the first mode-2 call of a ctx with a new window builds and uploads that
 * window's table; a ctx keeps six).  No atomics: the same bits every call. */
#define SSP_FEATNORM_TILE 256 /* frames of one utterance a workgroup takes: lengths around its multiples are the kernel's edge cases */
int ssp_featnorm_sliding(ssp_ctx* ctx, const float* feats, const ssp_segments* frame_seg, int32_t dim, int32_t window, int32_t mode,
                         float* out, int where, float* kernel_ms);
/* The rows of feats whose mask byte is non-zero, in order, packed from row 0 of out: utterance u's kept rows follow utterance u - 1's,
 * rows are copied bit for bit (NaN payloads included), rows of out past the total kept are not written.  mask: uint8[frames], indexed
 * like the rows of feats, on the side `where` names (any alignment); out: float[(frames of frame_seg) x dim], room for every row; counts_out:
 * HOST int64[n utterances], the kept rows of each, from which the caller builds the new segment table.  One host wait, for the
 * counts.  out == feats is SSP_ERR_INVALID, overlapping arrays are not supported.  What Kaldi's select-voiced-frames and sidekit's
 * label selection do (recalled, parity unpinned). */
int ssp_select_frames(ssp_ctx* ctx, const float* feats, const ssp_segments* frame_seg, int32_t dim, const uint8_t* mask, float* out,
                      int64_t* counts_out, int where, float* kernel_ms);
/* The warping table of a window, built on the host in double (no GPU, no ctx): row n (1 <= n <= window) holds
 * float(phi^-1(k / 2n)), k = 1 .. 2n - 1, at offset (n - 1)^2; the entry at k = n is exactly 0 and entry k is exactly the negative of
 * entry 2n - k.  table_out: HOST float[window * window]. */
int ssp_featnorm_table(int32_t window, float* table_out);

/* ---- PLP back end: replaces sidekit.frontend.features.plp after its power spectrum -> Bark bands -> ln stage (call sites
 * GMM_UBM.py:95, d_vector.py:93, UI/GMM_UBM_GUI.py:93, UI/tmp.py:315-318; that front stage is ssp_mfcc_run with a Bark table and
 * an identity DCT).  logspec: float[F x n_bands] ln critical-band energies laid out by frame_seg (which must start at frame 0);
 * rasta != 0: RASTA filtering along time per utterance (first four frames of an utterance come out as the flat-spectrum
 * cepstrum, as in rastamat); then equal-loudness (band centres 0..fmax_hz in Bark), ^0.33, autocorrelation, Levinson-Durbin of
 * order plp_order - 1, LPC -> cepstrum, lifter n^lift.  ceps_out: float[F x plp_order] (c0 first).  sidekit's source is absent
 * from the reference tree: the arithmetic follows the published rastamat algorithm it ports (parity unpinned). */
int ssp_plp_post(ssp_ctx* ctx, const float* logspec, const ssp_segments* frame_seg, int32_t n_bands, float fmax_hz,
                 int32_t plp_order, int32_t rasta, float lift, float* ceps_out, int where, float* kernel_ms);
/* ---- PLP feature recipes: everything the reference does to sidekit's PLP cepstra before a GMM sees them, in one call — GMM_UBM.py:94-99
 * (plp -> hstack(c, delta c) -> scale), UI/tmp.py:309-324 (per 1 s chunk: scale(plp), scale(hstack(mfcc, plp))), UI/GMM_UBM_GUI.py:85-100.
 * logspec, frame_seg, n_bands .. lift: as ssp_plp_post.  delta_order 0..2 appends the regression delta over +-2 frames (edge padded
 * inside the utterance, GMM_UBM.py:53-69) and the delta of it; scale != 0 standardises every PLP column per utterance as
 * sklearn.preprocessing.scale does (statistics over the entries that are not NaN, a deviation below 10 FLT_EPSILON counts as 1, NaN stays).
 * left: float[F x left_dim] columns finished elsewhere (the MFCC plan's output with cmvn = scale and the same delta_order), copied
 * unchanged; null / 0 for none; left_dim must be a multiple of 1 + delta_order.  feats_out: [F x (left_dim + (1 + delta_order) plp_order)]
 * float32 (out_type 0) or float64 (1, widened exactly), rows laid out for b = 0 .. delta_order as [left block b | PLP block b] with
 * left blocks of left_dim / (1 + delta_order) columns: scale(hstack(mfcc, plp, d mfcc, d plp)) at delta_order 1.
 * logspec, left and feats_out are all host or all device arrays (where); device arrays need only their natural alignment.  All work
 * is ordered on the ctx stream and a device-pointer call returns without a host wait (kernel_ms == NULL).  21 bands / order 13 and
 * 17 bands / order 13 run as one kernel, an utterance per workgroup, when the call's longest utterance fits 64 KiB of LDS (464 frames
 * at 21 bands, 336 with delta_order 2; 512 at most); any other size or a longer utterance chains the stand-alone kernels on the stream.  An empty
 * utterance writes nothing.  Limits as ssp_plp_post (SSP_ERR_UNSUPPORTED); bad arguments answer SSP_ERR_INVALID before any GPU work. */
int ssp_plp_features(ssp_ctx* ctx, const float* logspec, const ssp_segments* frame_seg, int32_t n_bands, float fmax_hz,
                     int32_t plp_order, int32_t rasta, float lift,
                     const float* left, int32_t left_dim,          /* may be null / 0 */
                     int32_t delta_order /* 0..2 */, int32_t scale /* 0 | 1 */,
                     void* feats_out, int out_type /* 0 float32 | 1 float64 */, int where, float* kernel_ms);

/* ---- voice activity detection: replaces VAD.py's per-frame Python loops (enframe VAD.py:28-50, energy :67-76, ZCR :53-64,
 *      spectrum_entropy :79-105, feature :108-119, the peak normalisation of wavdata :131) and its two detectors (VAD_detection
 *      :136-182, VAD_frequency :185-186) for a ragged batch of utterances ---- */
/* math.ceil(wlen / step) (VAD.py:37): the last frames run past the utterance's end and are zero padded.  No GPU. */
int ssp_vad_num_frames(int64_t n_samples, int32_t step, int64_t* n_frames);
/* frame segments (starting at frame 0) derived from sample segments with that rule */
int ssp_vad_frame_segments(ssp_ctx* ctx, const ssp_segments* sample_seg, int32_t step, ssp_segments** frame_seg_out);
/* feature (VAD.py:108-119) of every frame of every utterance in one pass: zcr_out = crossings * (power > 0.1), power_out = sum of squares,
 * entropy_out = spectral entropy of bins 0..127 in 10 blocks of 12 (VAD.py:79-92); float[total frames] each, laid out by frame_seg.
 * samples: sample_type 0 float32 | 1 int16 (taken at their integer value), laid out by sample_seg as ssp_mfcc_run takes them.  No window,
 * no pre-emphasis.  normalize != 0: every utterance is divided by its peak max|x| first (wavdata, VAD.py:131; int16 widened before the
 * abs: |-32768| = 32768); a digitally silent utterance (peak 0) gives NaN power and entropy and zcr 0, as the reference's 0 / 0 does.
 * normalize == 0: the samples are taken as they are (the caller's frames are already in [-1, 1]).  flags: SSP_VAD_ZCR_UNGATED makes
 * zcr_out the bare count of ZCR (VAD.py:53-64), without the power gate; other bits answer SSP_ERR_INVALID.  frame_size 256 with step 128 (the reference's frameSize / overlap) or step 256
 * (the columns of an enframe matrix handed over as one utterance); anything else answers SSP_ERR_UNSUPPORTED.  frame_seg must hold
 * ceil(n / step) frames per utterance.  where = SSP_HOST stages the batch whole.  One host wait per call, before the kernels are
 * queued (the upload of the call's chunk table). */
#define SSP_VAD_ZCR_UNGATED 1u
int ssp_vad_features(ssp_ctx* ctx, const void* samples, int sample_type, const ssp_segments* sample_seg, const ssp_segments* frame_seg,
                     int32_t frame_size, int32_t step, int32_t normalize, uint32_t flags, float* zcr_out, float* power_out, float* entropy_out, int where,
                     float* kernel_ms);
/* mode 0: VAD_detection(zcr, power, zcr_gate, ampl, amph) (VAD.py:136-182) per utterance of frame_seg, min_len = 16 in the reference
 * (>= 1): a frame with power > amph extends the current run and opens one if none is open; any other frame flushes a run longer than
 * min_len — start walks back and end forward while power > ampl or zcr > zcr_gate, [start, end] is marked — and leaves a shorter one
 * OPEN (a later loud frame extends it across the gap); a run open at the last frame is never flushed.  The reference's last_end /
 * min_distance merge can never be taken and is not implemented.  The backward walk stops at frame 0 (Python's index -1 would go on with
 * the last frame: the same result whenever the last frame is not active).
 * mode 1: VAD_frequency (VAD.py:185-186) on the entropy plane: 0 where entropy > ampl (0.4 in the reference), else 1; zcr, zcr_gate, amph
 * and min_len are not read.
 * mask_out: uint8[total frames]; n_speech_out (nullable): int32[n utterances] = marked frames per utterance. */
int ssp_vad_detect(ssp_ctx* ctx, const float* zcr, const float* power_or_entropy, const ssp_segments* frame_seg, int32_t mode, float zcr_gate,
                   float ampl, float amph, int32_t min_len, uint8_t* mask_out, int32_t* n_speech_out, int where, float* kernel_ms);
/* The objective of VAD.py's threshold search (optimize / cv, VAD.py:189-220) for n_par threshold sets in one launch: for every set j
 * and utterance u of frame_seg, counts_out[j][u][0..2] = tp, fp, fn = |mark & label|, |mark & ~label|, |~mark & label| over the
 * utterance's frames, where mark is exactly the mask ssp_vad_detect(mode, zcr_gate[j], ampl[j], amph[j], min_len) writes (same state
 * machine, same semantics: min_len a parameter, no last_end merge, the backward walk stops at frame 0) and label = (labels != 0).
 * F1 = 2 tp / (2 tp + fp + fn) (sklearn.metrics.f1_score, VAD.py:210); no mask leaves the device.
 * labels: uint8[total frames] laid out by frame_seg.  zcr_gate / ampl / amph: HOST arrays of n_par floats each, whatever `where` says
 * (NaN thresholds and NaN power are legal: their comparisons are false, as in the reference).  mode 1 (VAD_frequency with a list of
 * entropy thresholds, mark = !(entropy > ampl[j])) reads ampl only: zcr, zcr_gate and amph may be null, min_len must still be >= 1.
 * `where` applies to zcr / power_or_entropy / labels / counts_out.  Integer counts, no atomics: the result is deterministic.
 * SSP_ERR_INVALID: a null pointer that is needed, n_par < 1, min_len < 1, a bad mode or where.  SSP_ERR_UNSUPPORTED, before any
 * launch: an utterance longer than 131072 frames (the word planes of one utterance live in 64 KiB of LDS), or counts_out larger than
 * 2^31 entries.  One host wait per call, before the kernel is queued (the upload of the threshold arrays). */
int ssp_vad_sweep(ssp_ctx* ctx, const float* zcr, const float* power_or_entropy, const uint8_t* labels, const ssp_segments* frame_seg,
                  int32_t mode, int32_t n_par, const float* zcr_gate, const float* ampl, const float* amph, int32_t min_len,
                  int32_t* counts_out /* [n_par][n_utt][3] tp, fp, fn */, int where, float* kernel_ms);

/* ---- GMM-UBM scoring: replaces the GMM[i].score(x_j) - UBM.score(x_j) double loop
 *      (GMM_UBM.py:181-197) and sklearn GaussianMixture.score_samples/score for diag models ---- */
/* weights: HOST double[n_models x K]; means, covars: HOST double[n_models x K x D].
 * has_ubm != 0: model 0 is the UBM; argmax/score differences are taken over models 1..
 * Weights: every weight is finite and >= 0 and no model's weights are all zero; anything else (a negative, NaN or infinite weight, an
 * all-zero model) and a covariance that is not > 0 answer SSP_ERR_INVALID before anything is uploaded (the message names the model).  A
 * mixture of weight 0 does not exist, as in sklearn (log 0 = -inf inside the log-sum-exp): it is packed like a padded mixture and the
 * model's log-likelihoods are those of its other mixtures, at every precision. */
int ssp_gmm_pack(ssp_ctx* ctx, int32_t n_models, int32_t K, int32_t D, const double* weights,
                 const double* means, const double* covars, int32_t has_ubm, ssp_gmm** out);
int ssp_gmm_destroy(ssp_gmm* gmm);
/* feats: float[total frames x D]; loglik_out (nullable): float[n_models x total frames] (model-major,
 * = score_samples per model); scores_out (nullable): float[n_utt x n_models] mean log-likelihood
 * (= GaussianMixture.score); argmax_out (nullable): int32[n_utt] = argmax_i(score_i - score_ubm)
 * over speaker models (index 0 = first speaker model); precision: 0 fp32 MFMA (parity path) |
 * 1 bf16x3 split MFMA (fast path, same tolerance class) with every utterance whose top-2 margin lies inside the split-precision
 * error band scored again on the fp32 path, so the arg-max equals precision 0's | 2 bf16x3 split MFMA alone | 3 as 1 with the
 * calibrated band 8e-5 (|UBM score| + 1) (eight times the error measured at K = 64 / 512, D = 39): a HEURISTIC, about 100 times narrower
 * than 1's bound (rounding errors do not conspire and they average over an utterance's frames), so far fewer utterances are scored twice.
 * (precision 1: the band is a BOUND, not a calibration: with every operand split hi + lo the exponent of a mixture is off by at most
 *  eps * S(x), S(x) = sum_d |x_d| max|mu P|_d + x_d^2 max(P/2)_d (maxima over every mixture of every model, taken at ssp_gmm_pack),
 *  eps = 3.01 * 2^-18 + 8 D 2^-23 (the products a two-term split leaves out + worst-case fp32 accumulation on both paths); the
 *  log-sum-exp is 1-Lipschitz and the mean a mean, so a margin between two models is resolved when it exceeds
 *  2 (eps mean_t S(x_t) + 2^-20 (max_m |score_m| + 1)): gmm.hip gmm_band_kernel.  The call reads the flag count on the host, so it
 *  synchronises the stream even with device pointers and cannot be captured in a graph.  precision 0 is the parity path.
 *  What comes back for a close call (precision 1 / 3): the utterance's CANDIDATE models — those within the band of its best score, and
 *  the UBM — are scored again in fp32 and only THEIR entries of its scores_out row are replaced; the row's other entries keep their
 *  bf16x3 values (within the band of the fp32 path's).  The arg-max is the fp32 path's in every case.  A re-scoring pass too large for
 *  one launch scores every model and replaces the whole row.)
 * What precision 0 delivers: a mixture's exponent is evaluated EXPANDED, [x, x^2, 1] . W in fp32, so its error follows the size of the
 * expansion's terms (about D (|mu| / sigma)^2 per mixture), not the size of the result: at |mu| / sigma <= 1 the per-frame error is some
 * 1e-5 nats, on un-centred features it grows with (|mu| / sigma)^2 (measured per |mu| / sigma in profiles/gmm_accuracy.md) — a caller
 * whose features carry a large common offset subtracts it from the features and the means first (the model is translation invariant).
 * Without loglik_out the per-utterance means are formed inside the scoring kernel (the [n_models x frames] matrix never exists).  With
 * loglik_out the matrix is scored in ONE pass at the asked precision and scores_out / argmax_out are its per-utterance means: nothing is
 * listed or scored twice and there is no host wait at any precision (precision 1 / 3 then answer as 2, ssp_gmm_last_rescored is 0).
 * Non-finite rows.  A frame is BAD when any of its D entries is NaN or +-inf (the sidekit front end hands a digitally silent frame on as
 * a NaN row on purpose).  What the call does with one, at every precision (0 to 4), fed from the host, the device, in slices, in
 * scratch-bounded batches or through ssp_gmm_score_list:
 *   bad frame       loglik_out is NaN at that frame under EVERY model (never -inf: an infinite entry meets inf - inf in the exponent or
 *                   in the log-sum-exp's running maximum).
 *   bad utterance   (one that holds a bad frame) every entry of its scores_out row is NaN and its argmax_out is 0 — numpy.argmax of an
 *                   all-NaN row.  An empty utterance (T = 0) keeps the same NaN row and arg-max 0, the mean over no frames.
 *   everything else no other frame and no other utterance changes.  precision 0 / 2: the other columns of loglik_out and the other rows of
 *                   scores_out / argmax_out are BIT-IDENTICAL to those of the same call with the bad entries replaced by finite ones (same
 *                   layout).  precision 1 / 3 / 4: the arg-max is the same and the scores stay within the tolerance class; the set of
 *                   listed utterances changes (below) and with it a clean listed utterance's place in the compact re-scoring matrix.
 *   listing         precision 1 / 3 (calls without loglik_out: those with it list nothing) always list a bad utterance (its margin is
 *                   not comparable), score it again under every model, and count it in ssp_gmm_last_rescored.
 * The call itself stays IEEE and reports no error for such rows; the sklearn-shaped Python layer (gmm_train.GaussianMixture,
 * GMM_UBM.score_matrix) raises ValueError, as sklearn's input validation does. */
int ssp_gmm_score(ssp_gmm* gmm, const float* feats, const ssp_segments* frame_seg, float* loglik_out,
                  float* scores_out, int32_t* argmax_out, int where, int precision, float* kernel_ms);
/* ssp_gmm_score_list: the scoring loops GMM_UBM.py:181-197 on a LIST of per-utterance feature matrices, without the host's vstack and
 * astype.  rows: HOST array of n pointers (n = frame_seg's count) to (T_u x dim) row-major matrices of row_type 0 float32 | 1 float64
 * (narrowed to float32 on the host, round to nearest, as numpy's astype does); T_u from frame_seg, which starts at frame 0 and belongs
 * to the gmm's ctx; a null pointer only for T_u = 0.  dim: the D the gmm was packed with (the caller's promise, as feats' size is
 * ssp_gmm_score's).  Worker threads gather the rows into a pinned buffer kept on the ctx; ssp_gmm_score(SSP_HOST) then scores it:
 * scores_out / argmax_out as there, bit for bit, every precision.  A bad argument answers SSP_ERR_INVALID before any GPU work. */
int ssp_gmm_score_list(ssp_gmm* gmm, const void* const* rows, int row_type, int32_t dim, const ssp_segments* frame_seg,
                       float* scores_out, int32_t* argmax_out, int precision, float* kernel_ms);
/* utterances the last ssp_gmm_score / ssp_gmm_score_list call scored again on the fp32 path (diagnostics): the close calls of
 * precision 1 / 3 (and of 4 when it ran as 1), bad and empty utterances among them; 0 after a call at precision 0 / 2 or with loglik_out */
int ssp_gmm_last_rescored(const ssp_gmm* gmm, int32_t* n_out);
/* precision = 4 (auto; GMM_UBM.py:183-187's arg-max with the fp32 path's result on every utterance, never dearer than the cheaper of the
 * two ways to get it): precision 1's guarantee scores close calls twice, which costs more than precision 0 once most utterances are
 * close calls.  A pilot — split-precision pass, band and candidate lists on the first ~2 % of the utterances (>= 256) — prices the
 * re-scoring (listed frames x candidate models); the call then runs as precision 1 when that predicts less than the fp32 pass, else as
 * precision 0.  Batches of fewer than ~16 machine-filling rounds of frames (3.1 M at 256 CUs) skip the pilot — it would cost a round of
 * its own — and decide LATE: the split pass runs on everything and, when re-scoring the close calls it lists would cost more than a
 * whole fp32 pass, that pass runs instead (at worst 1.33 x the fp32 path).  Batches under 1024 utterances and calls that ask for
 * loglik_out run as precision 0.  One extra host wait.
 * ssp_gmm_last_auto: what the last such call chose (precision_used; -1: none yet) and saw (predicted_cost: of precision 1, in units of
 * the fp32 pass). */
int ssp_gmm_last_auto(const ssp_gmm* gmm, int32_t* precision_used, int32_t* pilot_utts, int32_t* pilot_listed, float* predicted_cost);

/* ---- GMM training (EM): the O(frames x K x D) part of one iteration of sklearn GaussianMixture(covariance_type='diag').fit as
 *      the reference trains its speaker models and UBM (GMM_UBM.py:158-170; sklearn mixture/_base.py:_e_step,
 *      mixture/_gaussian_mixture.py:_estimate_gaussian_parameters) ---- */
/* Current parameters: HOST double weights[K], means[K x D], covars[K x D].  feats: float[n_frames x D].
 * Outputs (HOST double): nk_out[K] = sum_t resp[t,k];  sx_out[K x D] = sum_t resp[t,k] x[t,d];  sxx_out[K x D] = sum_t resp[t,k] x[t,d]^2;
 * loglik_sum_out = sum_t logsumexp_k(log w_k + log N(x_t | k))  (n_frames x sklearn's lower bound of the E step).
 * The O(K x D) closing arithmetic of the M step and the convergence test stay with the caller (float64).
 * Non-finite rows.  When any of the n_frames rows holds a NaN or +-inf entry (a BAD frame, as for ssp_gmm_score), EVERY entry of nk_out,
 * sx_out and sxx_out and loglik_sum_out are NaN, on each kernel family (D <= 47 with K <= 64 or K > 64, D > 47); the call reports no
 * error, and nothing of it stays behind in the ctx's scratch: the next call on clean rows gives the bits it gave before.  A caller that
 * iterates (gmm_train.GaussianMixture.fit) must look before it loops: |NaN - previous bound| < tol never holds.
 * Accuracy (this call, ssp_gmm_em_stats_batch and ssp_gmm_em_stats_shared alike).  The kernels evaluate the EXPANDED quadratic
 * lp = c + sum_d x_d (mu_d P_d - x_d P_d / 2) in float32 and resp = exp(lp - lse) from it; the sums over the frames are float32 per
 * workgroup and float64 across them.  The error of a statistic is proportional to the SUM OF THE MAGNITUDES of the terms, not to their
 * sum: a few float32 roundings of sum_d (|x mu P| + x^2 P / 2) + |c| nats on every exponent, and that many parts of every
 * responsibility.  On centred features (|mu| / sigma of order 1) that is 1e-6 .. 1e-5 of a mixture's mass.  A common offset of r sigma
 * in every column makes the terms r^2 larger than their sum: measured 2e-4 relative on nk / sx / sxx at r = 10, 3e-3 at r = 30 and
 * 2e-2 at r = 100, with 0.07 nat per frame on loglik_sum there (D = 13 .. 39, overlapping mixtures, mixtures holding at least one
 * frame; profiles/em_accuracy.md).  Centre the features (subtract a global mean) before training on raw cepstra; the library does
 * not do it for the caller.  tests/em_cases.py holds every kernel to 8 x the error of a plain float32 restatement of this formula, on
 * and off centre. */
int ssp_gmm_em_stats(ssp_ctx* ctx, int32_t K, int32_t D, const double* weights, const double* means, const double* covars,
                     const float* feats, int64_t n_frames, double* nk_out, double* sx_out, double* sxx_out,
                     double* loglik_sum_out, int where, float* kernel_ms);

/* The same statistics for M models in one call (one EM iteration of many speaker models; GMM_UBM.py:154-170 trains one per speaker).
 * Model m is scored over rows [row_off[m], row_off[m] + n_frames[m]) of feats (float[n_rows x D], on the side `where` names); the ranges
 * may come in any order, leave gaps and overlap.  HOST double weights[M x K], means[M x K x D], covars[M x K x D]; outputs (HOST double)
 * nk_out[M x K], sx_out / sxx_out[M x K x D], loglik_sum_out[M], each model's as ssp_gmm_em_stats defines them.  row_off / n_frames:
 * HOST int64[M].  SSP_ERR_INVALID: M < 1, a model without frames, a range outside [0, n_rows), a non-positive weight or covariance
 * (the messages name the model).  SSP_ERR_UNSUPPORTED: D > 47.
 * Contract.  K <= 64: each model's outputs are BIT-IDENTICAL to ssp_gmm_em_stats on that model's rows (same kernel body, same partition
 * of its frames, same float64 reduction order).  K > 64: fp32 MFMA log-sum-exp per frame and fp32 partial sums reduced in float64, within
 * fp32 rounding of ssp_gmm_em_stats (whose per-frame log-sum-exp is the same kernel body's; only the partition of the frames among the
 * persistent workgroups differs) but not bit for bit.
 * Non-finite rows.  A model whose row range holds a bad frame gets NaN in all of its nk_out, sx_out, sxx_out and loglik_sum_out, as
 * ssp_gmm_em_stats gives.  A model whose range holds none is BIT-IDENTICAL to the same call without the bad entries — whichever other
 * models of the launch are poisoned, overlapping ranges included — and a bad frame in a gap between the ranges, or in the rows of a
 * model's last 64-frame tile that lie past its range, is never read.
 * Work: one upload of the parameters and one result copy + host wait per call; the models' partial sums are grouped into launches under
 * a scratch budget (SSP_EM_BATCH_SCRATCH_MB, default 1024). */
int ssp_gmm_em_stats_batch(ssp_ctx* ctx, int32_t M, int32_t K, int32_t D, const double* weights, const double* means,
                           const double* covars, const float* feats, int64_t n_rows, const int64_t* row_off, const int64_t* n_frames,
                           double* nk_out, double* sx_out, double* sxx_out, double* loglik_sum_out, int where, float* kernel_ms);

/* The same statistics of M row ranges under ONE shared model: what MAP adaptation of a universal background model needs per speaker
 * (Reynolds, Quatieri, Dunn 2000).  An EXTENSION: the reference trains every speaker's mixture independently (GMM_UBM.py:158-170) and
 * has no adaptation step.  HOST double weights[K], means[K x D], covars[K x D]: one parameter block, packed and uploaded once and read by
 * every range (the batched kernels with a parameter stride of 0).  Everything else as ssp_gmm_em_stats_batch: feats, row_off, n_frames,
 * the outputs nk_out[M x K], sx_out / sxx_out[M x K x D], loglik_sum_out[M], the error codes and the non-finite-row rules.
 * Contract.  Every output is BIT-IDENTICAL to ssp_gmm_em_stats_batch called with the parameters repeated M times, for K <= 64 and
 * K > 64 alike (same kernels, same partition, same reduction order). */
int ssp_gmm_em_stats_shared(ssp_ctx* ctx, int32_t M, int32_t K, int32_t D, const double* weights, const double* means,
                            const double* covars, const float* feats, int64_t n_rows, const int64_t* row_off, const int64_t* n_frames,
                            double* nk_out, double* sx_out, double* sxx_out, double* loglik_sum_out, int where, float* kernel_ms);

/* ---- Full-covariance GMMs: sklearn GaussianMixture(covariance_type='full'), sklearn's default.  An EXTENSION: the reference's two call
 *      sites (GMM_UBM.py:158,169) train 'diag' models; a pickled sklearn model of the default type, and the full-covariance UBMs the
 *      i-vector / PLDA / diarization chains usually start from, are scored and trained here. ----
 * Definitions (sklearn mixture/_gaussian_mixture.py).  A model is HOST double weights[K], means[K x D] and prec_chol[K x D x D], row-major:
 * sklearn's precisions_cholesky_, U_k = solve_triangular(cholesky(Sigma_k, lower=True), I, lower=True).T, UPPER triangular
 * (_compute_precision_cholesky); only the upper triangle is read.  Per frame x_t (_estimate_log_gaussian_prob, _estimate_log_prob_resp):
 *   y_tk = (x_t - mu_k) U_k;  lp_tk = log w_k - 1/2 (D log 2 pi + sum_j y_tkj^2) + sum_j log U_kjj;  lse_t = logsumexp_k lp_tk;
 *   resp_tk = exp(lp_tk - lse_t).
 * ssp_gmm_full_em_stats: the sums of one EM iteration (_estimate_gaussian_parameters, _estimate_gaussian_covariances_full in raw-moment
 * form) about a caller-given shift c (HOST double[D]; null = 0), x' = x - c:
 *   nk_out[K] = sum_t resp_tk;  sx_out[K x D] = sum_t resp_tk x'_t;  sxx_out[K x D x D] = sum_t resp_tk x'_t x'_t^T (exactly symmetric,
 *   both triangles written);  loglik_sum_out = sum_t lse_t.
 * The model is translation invariant: the shift only moves where float32 rounding happens (mu - c is formed in float64 on the host, the
 * kernels subtract c from every x as they load it).  A caller that passes the global mean (gmm_train does) has no need to centre its
 * features first.  The M step stays with the caller in float64: nk += 10 eps, m' = sx / nk, means = m' + c,
 * Sigma = sxx / nk - m' m'^T + reg_covar I, U by _compute_precision_cholesky.
 * feats float[n_frames x D] on the side `where` names (any 4-byte alignment); parameters and outputs are HOST arrays.
 * Limits: 1 <= D <= 64, K >= 1; outside that SSP_ERR_UNSUPPORTED (D) or SSP_ERR_INVALID before any launch.  SSP_ERR_INVALID before any
 * upload, the message naming model and mixture: a negative or non-finite weight, an all-zero weight vector, a diagonal entry of U that
 * is not finite and > 0, a non-finite entry in the upper triangle or the means.  A mixture of weight 0 does not exist (as in
 * ssp_gmm_pack): its responsibility is 0 and the other mixtures' results are the bits of the model without it.
 * Kernels: exact fp32 MFMA (v_mfma_f32_32x32x2_f32) in two passes, frames in slabs whose lp[K][slab] workspace respects
 * SSP_GMM_FULL_SCRATCH_MB (default 256).  Summation: one float32 accumulator adds at most 8192 frames (128 tiles of 64 per walker of the
 * moment pass; 256 per workgroup sum of lse); everything above that is added in float64 in a fixed order.  Deterministic: no
 * floating-point atomics, two calls on the same input give the same bits.
 * Non-finite rows, ssp_gmm_em_stats' rule: a BAD frame (a NaN or +-inf entry) makes EVERY entry of nk_out, sx_out, sxx_out and
 * loglik_sum_out NaN; no error is reported and nothing stays behind in the ctx's scratch: the next clean call gives the bits it gave
 * before.
 * ssp_gmm_full_pack / ssp_gmm_full_score: n_models models of K mixtures (weights[n_models x K], means[.. x D], prec_chol[.. x D x D]);
 * has_ubm: model 0 is the UBM.  Outputs as ssp_gmm_score's, each nullable, on the side `where` names: loglik_out float[n_models x F]
 * model-major (= score_samples), scores_out float[n_utt x n_models] per-utterance means (= score), argmax_out int32[n_utt] the arg-max
 * of score - UBM score over the speaker models (first index on ties).  One precision: exact fp32 MFMA.  Without loglik_out the means are
 * formed on the device from runs of whole utterances whose [n_models x frames] block fits SSP_GMM_FULL_SCRATCH_MB: the whole matrix
 * need not exist; scores_out is bit for bit the same with and without loglik_out.  Non-finite rows, ssp_gmm_score's rule: a bad frame is
 * NaN under every model (never -inf), its utterance's scores_out row is NaN and its argmax_out 0, and so are an empty utterance's; every
 * other frame and utterance is BIT-IDENTICAL to the same call with the bad entries replaced by finite ones.  Device-pointer calls queue
 * their kernels on the ctx stream and return without a host wait. */
int ssp_gmm_full_em_stats(ssp_ctx* ctx, int32_t K, int32_t D, const double* weights, const double* means, const double* prec_chol,
                          const double* shift, const float* feats, int64_t n_frames, double* nk_out, double* sx_out, double* sxx_out,
                          double* loglik_sum_out, int where, float* kernel_ms);
int ssp_gmm_full_pack(ssp_ctx* ctx, int32_t n_models, int32_t K, int32_t D, const double* weights, const double* means,
                      const double* prec_chol, int32_t has_ubm, ssp_gmm_full** out);
int ssp_gmm_full_destroy(ssp_gmm_full* gmm);
int ssp_gmm_full_score(ssp_gmm_full* gmm, const float* feats, const ssp_segments* frame_seg, float* loglik_out, float* scores_out,
                       int32_t* argmax_out, int where, float* kernel_ms);

/* ---- Top-C fast scoring of mean-adapted GMM-UBM speaker models (GMM_UBM.py:158-170,181-197 are what it stands beside).  An EXTENSION
 *      the reference does not have: its models are trained independently and its scoring loops evaluate every mixture of every one.
 *      For speaker models that share the UBM's weights and covariances and differ in their means (MAP adaptation of the means), the
 *      quantity of GMM_UBM.py:185, GMM[i].score(x) - UBM.score(x), is evaluated over the UBM's best C mixtures of every frame only. ----
 * Definition (quantities as sklearn mixture/_gaussian_mixture.py:453-512 defines them).  lp_k(x): the UBM's weighted log-probability of
 * mixture k at frame x.  T(x): the C mixtures of largest lp_k(x); of equal values the lower index ranks first.  For speaker s with means
 * mu_s: delta_{s,k}(x) = x . a_{s,k} - b_{s,k},  a_{s,k} = (mu_{s,k} - mu_k) P_k,  b_{s,k} = 1/2 sum_d (mu_{s,k,d}^2 - mu_{k,d}^2) P_{k,d}
 * (P = 1 / covariance; formed in float64 on the host, rounded to fp32).  L_ubm(x) = logsumexp_{k in T(x)} lp_k(x),
 * L_s(x) = logsumexp_{k in T(x)} (lp_k(x) + delta_{s,k}(x)).  Per utterance u:  diff[u][s] = mean_t (L_s(x_t) - L_ubm(x_t)),
 * ubm[u] = mean_t L_ubm(x_t).  With C = K (no zero weights) diff is the dense score difference exactly; the common part lp_k enters
 * only as the posterior of k within T(x), so its rounding error largely cancels.
 * ssp_gmm_map_pack: HOST double ubm_weights[K], ubm_means[K x D], ubm_covars[K x D], spk_means[S x K x D].  Validation as
 * ssp_gmm_pack: weights finite and >= 0 and not all zero, covariances > 0, else SSP_ERR_INVALID before anything is uploaded; a mixture
 * of weight 0 does not exist and is never selected.  SSP_ERR_INVALID: S < 1, K < 1, D < 1.  SSP_ERR_UNSUPPORTED: D > 47 (the selection
 * kernel's MFMA tiling, as ssp_gmm_em_stats_batch), a K whose bucket table outgrows the LDS.
 * ssp_gmm_map_score: feats float[total frames x D] (any 4-byte alignment) and frame_seg as ssp_gmm_score.  C: mixtures kept per frame.
 * Outputs (each nullable, on the side `where` names): diff_out float[n_utt x S]; ubm_out float[n_utt]; argmax_out int32[n_utt], the
 * FIRST index of the row's maximum (numpy.argmax); idx_out int32[total frames x C], T(x) of every frame in rank order.
 * SSP_ERR_INVALID, each found before any GPU work: C < 1, C larger than the number of non-zero-weight mixtures.  SSP_ERR_UNSUPPORTED:
 * C > 8.  The handle and its ctx stay usable after either.
 * Non-finite rows, as ssp_gmm_score states them: a BAD frame (a NaN or +-inf entry) makes its utterance's diff_out row and ubm_out NaN
 * and its argmax_out 0; its idx_out row is -1.  An empty utterance (T = 0) has the same NaN row, NaN ubm_out and arg-max 0.  Every other
 * utterance is BIT-IDENTICAL to the same call with the bad entries replaced by finite ones.  No error is reported; the Python layer
 * raises ValueError.
 * Deterministic: no floating-point atomics, every sum has a fixed shape, the same call gives the same bits every time, and an
 * utterance's results do not depend on the other utterances of the batch.  Stream-ordered: with device pointers the call queues its
 * kernels on the ctx stream and returns without a host wait; where = SSP_HOST stages the features whole and waits for the results.
 * Accuracy: lp_k is evaluated expanded in fp32 as ssp_gmm_score's precision 0 does (some 1e-5 nats per frame at |mu| / sigma <= 1):
 * two mixtures whose lp differ by less than that may swap ranks at the edge of T(x).
 * ssp_gmm_map_score_list: the same on a LIST of per-utterance matrices, gathered as ssp_gmm_score_list gathers them (rows, row_type, dim
 * and frame_seg as there; outputs HOST). */
int ssp_gmm_map_pack(ssp_ctx* ctx, int32_t K, int32_t D, const double* ubm_weights, const double* ubm_means, const double* ubm_covars,
                     int32_t S, const double* spk_means, ssp_gmm_map** out);
int ssp_gmm_map_destroy(ssp_gmm_map* map);
int ssp_gmm_map_score(ssp_gmm_map* map, const float* feats, const ssp_segments* frame_seg, int32_t C, float* diff_out, float* ubm_out,
                      int32_t* argmax_out, int32_t* idx_out, int where, float* kernel_ms);
int ssp_gmm_map_score_list(ssp_gmm_map* map, const void* const* rows, int row_type, int32_t dim, const ssp_segments* frame_seg, int32_t C,
                           float* diff_out, float* ubm_out, int32_t* argmax_out, int32_t* idx_out, float* kernel_ms);

/* ---- i-vector extraction and the E-step of total-variability training (Dehak et al. 2011, after Kenny 2005).  An EXTENSION and
 *      UNPINNED: the reference has no factor analysis; sidekit, the package it imports its features from, ships this model as
 *      FactorAnalyser.total_variability / extract_ivectors.  The yardstick is a float64 restatement (tests/ivector_oracle.py).  It joins
 *      the two scoring halves: ssp_gmm_em_stats_shared's statistics go in, a fixed-length embedding comes out, and that is what
 *      ssp_centroids / ssp_cosine_identify / ssp_l2_normalize take. ----
 * Definition.  A diagonal UBM with means mu (K x D) and covariances cv (K x D), a total-variability matrix T (K x D x R), and per
 * utterance u the statistics nk[u] (K) and sx[u] (K x D) as ssp_gmm_em_stats_shared returns them:
 *   f[u,k,:] = sx[u,k,:] - nk[u,k] mu[k,:]          (formed in float64, then rounded to fp32 once: sx and nk mu cancel)
 *   P_k = T_k' diag(1/cv_k) T_k  (R x R),   G = diag(1/cv) T  (K D x R)          (float64, rounded once)
 *   L_u = I + sum_k nk[u,k] P_k,   b_u = G' f_u,   w_u = L_u^-1 b_u  (the i-vector),   logdet_u = log|L_u|,   quad_u = b_u' w_u
 *   objective of a batch = sum_u (-logdet_u / 2 + quad_u / 2): the marginal log-likelihood up to a constant in T; EM never decreases it
 *   E-step accumulators  A_k = sum_u nk[u,k] (L_u^-1 + w_u w_u'),   C = sum_u f_u w_u'  (K x D x R);   M-step (the caller's)  T_k = C_k A_k^-1
 * No covariance update, no minimum-divergence step.  The back end (LDA, length normalisation, PLDA) is the ssp_plda block below.
 * Every array is a HOST array: the statistics arrive on the host from ssp_gmm_em_stats_shared (device-resident statistics are a
 * follow-up).  ubm_means / ubm_covars double[K x D], T double[K x D x R]; nk double[U x K], sx double[U x K x D]; w_out float[U x R],
 * logdet_out / quad_out float[U] (nullable); A_out double[K x R x R] (full, symmetric), C_out double[K x D x R], objective_out (nullable).
 * SSP_ERR_INVALID, each found before any GPU work: K, D, R or U < 1, a covariance that is not positive and finite, a non-finite T or
 * mean.  SSP_ERR_UNSUPPORTED: R > 256 (the packed triangle of L_u lives in one workgroup's LDS).  The ctx stays usable after either.
 * Work per call: the device is fp32 with exact-fp32 MFMA.  sum_k nk P_k is one GEMM against the K packed lower triangles of P (row i,
 * column j <= i at i (i + 1) / 2 + j), b one GEMM against G; one workgroup per utterance then factors L_u in LDS (Cholesky), solves,
 * and for the E-step goes on in place to L_u^-1; the accumulators are two more GEMMs (N' S and f' W).  ssp_ivector_set_t re-packs P
 * and G on the device from the uploaded float64 T.  A large batch runs in slabs of whole utterances under the workspace cap
 * (ssp_ivector_set_workspace, default 1 GiB, counts what grows with the slab; one utterance always runs; ssp_ivector_last_slab: the
 * utterances per slab of the last call); the E-step's accumulators are added over the slabs in slab order in float64.
 * Contracts.  An utterance's w_out, logdet_out and quad_out bits do not depend on U, on the slab size or on its place in the batch.
 * An utterance with every nk = 0 (and sx = 0) gives w = 0, logdet = 0, quad = 0 exactly.  No floating-point atomics, every sum has a
 * fixed shape: the same call gives the same bits every time.
 * Non-finite statistics.  An utterance whose nk or sx holds a non-finite entry (or one too large for fp32) gives NaN in its own w_out,
 * logdet_out and quad_out only; every other utterance is BIT-IDENTICAL to the same call with that utterance's statistics replaced by
 * zeros.  ssp_ivector_estep on such a batch returns NaN accumulators and a NaN objective.  No error is reported; the Python layer
 * raises ValueError naming the utterance.
 * kernel_ms: the device time of the kernels, copies excluded; ssp_ivector_last_stages then holds its split, float[5]: the precision
 * GEMM, the right-hand-side GEMM, the Cholesky kernel, and for the E-step the A and the C accumulator GEMMs. */
int ssp_ivector_create(ssp_ctx* ctx, int32_t K, int32_t D, int32_t R, const double* ubm_means, const double* ubm_covars,
                       const double* T, ssp_ivector** out);
int ssp_ivector_destroy(ssp_ivector* iv);
int ssp_ivector_set_t(ssp_ivector* iv, const double* T);
int ssp_ivector_set_workspace(ssp_ivector* iv, size_t bytes);
int ssp_ivector_last_slab(const ssp_ivector* iv, int64_t* utterances);
int ssp_ivector_last_stages(const ssp_ivector* iv, float* ms);
int ssp_ivector_extract(ssp_ivector* iv, const double* nk, const double* sx, int64_t U, float* w_out, float* logdet_out, float* quad_out,
                        float* kernel_ms);
int ssp_ivector_estep(ssp_ivector* iv, const double* nk, const double* sx, int64_t U, double* A_out, double* C_out, double* objective_out,
                      float* kernel_ms);

/* ---- PLDA back end for fixed-length embeddings: class statistics, and log-likelihood-ratio scoring of a diagonalised two-covariance
 *      model (Ioffe 2006; Prince & Elder 2007; the two-covariance form of Sizov, Lee & Kinnunen 2014; EM after Kaldi's PldaEstimator;
 *      length normalisation after Garcia-Romero & Espy-Wilson 2011).  An EXTENSION and UNPINNED: the reference has no back end; sidekit
 *      and Kaldi ship this chain.  The yardstick is a float64 restatement (tests/plda_oracle.py).  It ends the chain that
 *      ssp_ivector_extract and the d-vector networks begin: embeddings go in, speaker log-likelihood ratios come out. ----
 * Model.  x = mu + y_s + e,  y_s ~ N(0, B),  e ~ N(0, W);  vectors of dimension q.
 * Class statistics of rows X (N x q) with labels in [0, S)   (ssp_plda_stats):
 *   n_s = rows of speaker s;   sum_s = their sum, in float64 IN ROW ORDER (as ssp_centroids);   m_s = sum_s / n_s   (float64)
 *   mu = (sum_0 + sum_1 + ... + sum_{S-1}) / N, the class sums added in ascending s in float64: the mean of all rows
 *   S_w = sum_i (x_i - m_{s(i)}) (x_i - m_{s(i)})':  each row is centred in float64 and rounded to fp32 ONCE; S_w is then a transposed-A
 *   GEMM on exact-fp32 MFMA in k-chunks of 1024 rows, each chunk ONE k-ordered chain, the chunks added in float64 in ascending order.
 *   A class without rows has count 0 and a zero sum and takes no part in S_w.  No floating-point atomics: same call, same bits.
 * EM (the caller's, on the host in float64; speech_signal_processing_amd/plda.py) needs only S_w, m_s and n_s.  From W = B = I, per
 * iteration, with the classes grouped by their distinct count c (k_c classes):  F_c = sum_{s: n_s = c} (m_s - mu)(m_s - mu)',
 *   V_c = (B^-1 + c W^-1)^-1,  G_c = c V_c W^-1,  H_c = I - G_c,
 *   B <- [sum_c (k_c V_c + G_c F_c G_c')] / S,    W <- [S_w + sum_c c (k_c V_c + H_c F_c H_c')] / N
 *   objective (of the W, B the iteration started from; EM never decreases it)
 *     = sum_s -1/2 [(n_s - 1) log|W| + log|B + W/n_s| + (m_s - mu)' (B + W/n_s)^-1 (m_s - mu)] - 1/2 tr(W^-1 S_w)
 * Diagonalisation.  W = L L' (Cholesky);  L^-1 B L^-T = U diag(psi) U', psi descending;  A = U' L^-1, so A W A' = I and
 *   A B A' = diag(psi).  Sign: the largest-magnitude entry of each row of A is positive.
 * Scoring.  With e_s = A (m_s^enrol - mu) the transformed mean of n_s enrolment vectors and t = A (x - mu):
 *   mean_{s,d} = n_s psi_d e_{s,d} / (n_s psi_d + 1),    var_{s,d} = 1 + psi_d / (n_s psi_d + 1)
 *   LLR(t, s) = -1/2 sum_d [log var_{s,d} + (t_d - mean_{s,d})^2 / var_{s,d}] + 1/2 sum_d [log(1 + psi_d) + t_d^2 / (1 + psi_d)]
 *   packed (ssp_plda_pack, float64 rounded once):  LLR = sum_d beta_{s,d} t_d - 1/2 sum_d alpha_{s,d} t_d^2 + c_s,
 *   beta = mean / var,   alpha = 1 / var - 1 / (1 + psi),   c_s = -1/2 sum_d [log var - log(1 + psi) + mean^2 / var]
 *   alpha depends on s only through n_s: speakers with the same count share one alpha row (G distinct counts).
 * LDA (optional, before PLDA; the caller's, float64): the top p <= min(q, S - 1) generalised eigenvectors of S_b v = lambda S_w v,
 *   S_b = sum_s n_s (m_s - mu)(m_s - mu)', normalised to v' S_w v = 1, the sign convention of A.
 * Length normalisation x <- x / |x| comes after centring and LDA and before A.  Centring, projection and normalisation need no entry
 *   point of their own: ssp_dense_forward (weights = the projection P, bias = -P mu) and ssp_l2_normalize.
 *
 * ssp_plda_stats.  X float[N x q], labels int32[N] on the side `where` names (any 4-byte alignment); N >= 1, 1 <= q <= 256 (else
 *   SSP_ERR_UNSUPPORTED), S >= 1.  The outputs are HOST arrays: sum_out double[S x q], count_out int64[S], mean_out double[q] (mu),
 *   sw_out double[q x q], full and EXACTLY symmetric.  A label outside [0, S): SSP_ERR_INVALID (found on the device; nothing is
 *   written).  A non-finite row is not singled out: the outputs are then non-finite, and the Python layer raises ValueError naming the
 *   row.  With device pointers the kernels queue on the ctx stream; the outputs being host arrays, the call waits ONCE at its end.
 * ssp_plda_pack.  psi double[q], enrol_mean double[S x q] ALREADY transformed by A, enrol_count int32[S] (HOST arrays).  Forms beta,
 *   -alpha / 2 and c in float64, rounds each once, lays beta out as MFMA tile images of 32 speakers (cos_pack_kernel's layout),
 *   de-duplicates alpha into G class rows and a per-speaker class index.  SSP_ERR_INVALID before any GPU work: q or S < 1, a count < 1,
 *   psi not finite or < 0, a non-finite mean.  SSP_ERR_UNSUPPORTED: q > 256.  flags bit 0 (SSP_PLDA_NO_CLASS_PATH): never use the
 *   class-shared path below.
 * ssp_plda_info.  What the pack decided: the number G of distinct enrolment counts, and whether ssp_plda_score takes the class-shared path.
 * ssp_plda_score.  T float[N x q], ALREADY transformed, on the side `where` names (any 4-byte alignment); llr_out float[N x S]
 *   (nullable), argmax_out int32[N], max_out float[N] (each nullable).  A wave keeps its 32 test vectors in registers as the MFMA B
 *   operand; speaker tiles stream through an LDS ring by LDS-DMA; v_mfma_f32_32x32x2_f32, one k-ordered chain per output; the
 *   epilogue adds c_s and keeps a running (max, first index).  The t^2 term: (a) class-shared, G <= 32: ONE tile of the G alpha rows
 *   against the squared operand first, parked in a 4 KiB per-wave LDS table that every speaker's epilogue reads at its class; (b)
 *   general, any G: every speaker tile is followed by its alpha tile against the squared operand into the same accumulator.  Both meet
 *   the same tolerance; they are not bit-equal to each other.
 *   Contracts.  A row's llr_out, argmax_out and max_out bits depend on neither N nor the row's place in the batch.  Arg-max ties go
 *   to the first index; max_out is llr[argmax] bit for bit.  A test row with a non-finite entry gives NaN in its own llr_out row and
 *   in max_out, and -1 in argmax_out; every other row is BIT-IDENTICAL to the same call with that row replaced by zeros.  No atomics
 *   on floats.  With device pointers the call is stream-ordered and never waits on the host; SSP_HOST stages the inputs and waits for
 *   the results.  N == 0 is a no-op.  kernel_ms: device time of the kernels, copies excluded (asking for it waits). */
#define SSP_PLDA_NO_CLASS_PATH 1
int ssp_plda_stats(ssp_ctx* ctx, const float* X, const int32_t* labels, int64_t N, int32_t q, int32_t S, double* sum_out,
                   int64_t* count_out, double* mean_out, double* sw_out, int where, float* kernel_ms);
int ssp_plda_pack(ssp_ctx* ctx, int32_t q, const double* psi, int32_t S, const double* enrol_mean, const int32_t* enrol_count,
                  int32_t flags, ssp_plda** out);
int ssp_plda_destroy(ssp_plda* plda);
int ssp_plda_info(const ssp_plda* plda, int32_t* n_classes, int32_t* class_shared);
int ssp_plda_score(ssp_plda* plda, const float* T, int64_t N, float* llr_out, int32_t* argmax_out, float* max_out, int where,
                   float* kernel_ms);

/* ---- Score normalisation against a cohort (S-norm, adaptive S-norm, T-norm, Z-norm) and detection-error counts over a threshold
 *      grid, for any score matrix: ssp_plda_score's ratios, 1 - ssp_cosine_identify's distances.  An EXTENSION and UNPINNED: the
 *      reference has neither (its only open-set decision is a fixed cosine threshold); Kaldi, sidekit, SpeechBrain and wespeaker ship
 *      both.  The yardstick is a restatement (tests/snorm_oracle.py).  Added to ABI 4 without a version step. ----
 * ssp_topn_stats.  scores float[rows x cols], row-major with leading dimension ld >= cols, on the side `where` names (any 4-byte
 *   alignment).  axis = 1: one result per row, over its cols entries; axis = 0: one result per column, over its rows entries (read at
 *   stride ld).  For a line of length L let m = min(n, L) and v_1 >= ... >= v_m its m largest entries as a multiset (ties make the set
 *   of indices ambiguous, not the values):
 *     kth = v_m, bit for bit an entry of the line (-0.0 and +0.0 compare equal: either may be returned)
 *     mean = kth + (1/m) sum_i (v_i - kth)          std = sqrt((1/m) sum_i (v_i - mean)^2)   (population form; the square sum is
 *     taken about the mean in a second pass, never as E[v^2] - mean^2; a constant line has std exactly 0)
 *   One wave per line: order-preserving 32-bit keys, the m-th largest key by bisection over the 32 key bits (exact), then sums of a
 *   fixed shape in fp32 (lane l adds entries l, l + 64, ... in that order, then a butterfly over the lanes; the copies of kth that
 *   complete the multiset are added last).  Lines up to 4096 entries stay in registers, longer ones are read again per pass.
 *   mean_out, std_out, kth_out float[rows] (axis 1) or float[cols] (axis 0), each nullable.
 *   A line with a non-finite entry gives NaN in its own mean, std and kth; every other line is BIT-IDENTICAL to the same call with
 *   that line replaced by zeros.  A line's bits depend on neither the number of lines nor its place.  No atomics: same call, same bits.
 *   SSP_ERR_INVALID before any GPU work: n < 1, rows < 0, cols < 1, ld < cols, axis not 0 or 1.  SSP_ERR_UNSUPPORTED: lines longer
 *   than 65536 (cols for axis 1, rows for axis 0).  rows == 0 is a no-op.
 * ssp_snorm_apply.  scores float[N x S] (ld >= S).  In fp32, operation by operation, IEEE division, no contraction:
 *     z[t,s] = 0.5f * ((x - col_mean[s]) / max(col_std[s], std_floor) + (x - row_mean[t]) / max(row_std[t], std_floor))
 *   row_mean / row_std float[N] are the test side (T-norm), col_mean / col_std float[S] the enrolment side (Z-norm); either PAIR may be
 *   NULL, the other term is then the whole result without the 0.5.  Both NULL, or half a pair: SSP_ERR_INVALID.  std_floor must be
 *   finite and > 0.  max is numpy's: a NaN deviation gives NaN.  out float[N x S] (ld_out >= S; nullable) may be `scores` itself with
 *   ld_out == ld.  argmax_out int32[N], max_out float[N] (each nullable): over the entries of the row that are not NaN, ties to the
 *   first index, max_out = z[argmax] bit for bit; a row without such an entry gives -1 and NaN.  A NaN in one row's statistics touches
 *   that row only, one in a column's statistics that column only.  N == 0 is a no-op.
 * ssp_det_counts.  scores float[N x S] (ld >= S) and target int32[N] on the side `where` names: target[t] is the enrolled speaker row t
 *   belongs to, -1 for none (every trial of the row is then a non-target); anything else outside [0, S): SSP_ERR_INVALID (found on the
 *   device; nothing is written).  thresholds: HOST float[M], ascending and finite, 0 <= M <= 4096 (else SSP_ERR_INVALID before any GPU
 *   work).  Bin of a score: b(x) = #{j : thresholds[j] <= x} in [0, M] (numpy.searchsorted, side = "right").  Outputs, all HOST arrays:
 *   tar_hist / non_hist int64[M + 1]: target and non-target trials per bin; nan_count int64[2]: NaN scores (target, non-target), counted
 *   apart; range_out float[4]: minimum and maximum of the target scores that are not NaN, then of the non-target ones (+inf / -inf
 *   where there is none).  Thresholds and per-workgroup histograms sit in LDS (integer LDS adds), one 64-bit integer add per bin and
 *   workgroup follows: the counts are exact.  M = 0 gives the totals and the ranges only.
 * Contracts of all three, as ssp_plda_score: device pointers at any 4-byte alignment; with device pointers ssp_topn_stats and
 *   ssp_snorm_apply are stream-ordered and never wait on the host, ssp_det_counts (host outputs) waits ONCE at its end; SSP_HOST stages
 *   the inputs and waits for the results.  An error leaves the ctx usable.  kernel_ms: device time of the kernels, copies excluded
 *   (asking for it waits). */
int ssp_topn_stats(ssp_ctx* ctx, const float* scores, int64_t rows, int32_t cols, int64_t ld, int32_t axis, int32_t n, float* mean_out,
                   float* std_out, float* kth_out, int where, float* kernel_ms);
int ssp_snorm_apply(ssp_ctx* ctx, const float* scores, int64_t N, int32_t S, int64_t ld, const float* row_mean, const float* row_std,
                    const float* col_mean, const float* col_std, float std_floor, float* out, int64_t ld_out, int32_t* argmax_out,
                    float* max_out, int where, float* kernel_ms);
int ssp_det_counts(ssp_ctx* ctx, const float* scores, int64_t N, int32_t S, int64_t ld, const int32_t* target, const float* thresholds,
                   int32_t M, int64_t* tar_hist, int64_t* non_hist, int64_t* nan_count, float* range_out, int where, float* kernel_ms);

/* ---- Speaker diarization: the scores of all segment pairs of a recording and agglomerative hierarchical clustering (AHC) of them, for
 *      a batch of recordings ("who spoke when" for speakers that are not enrolled: Kaldi's diarization/ recipe — short windows, one
 *      embedding each, PLDA or cosine scores of all pairs, AHC to a threshold or a known speaker count).  An EXTENSION and UNPINNED:
 *      the reference has no diarization; Kaldi, sidekit, SpeechBrain and wespeaker ship it on the same chain.  The yardstick is a
 *      restatement (tests/diarize_oracle.py), corroborated by SciPy's linkage.  Added to ABI 4 without a version step. ----
 * Layout.  seg holds R recordings; recording r owns rows offsets[r] .. offsets[r + 1] of the embedding matrix, n_r of them.  Score
 *   matrices are packed: recording r's n_r x n_r row-major dense block starts at float offset sq_off[r] = sum_{k < r} n_k^2.
 *   ssp_pairwise_size returns sum_r n_r^2.
 * ssp_pairwise_scores.  X float[offsets[R] x q] on the side `where` names; g, h HOST float[q] (NULL: ones / zeros).  For i, j of the
 *   same recording:   S[i,j] = sum_d g_d x_id x_jd - (r_i + r_j) + c0,   r_i = sum_d h_d x_id^2.
 *   Cosine: g = h = NULL, c0 = 0 on rows that went through ssp_l2_normalize.  PLDA: with the diagonalised model's psi and ONE enrolment
 *   vector (n_s = 1 in the scoring formulas above) the log-likelihood ratio of two projected vectors is symmetric and has this form with
 *     g = psi / (2 psi + 1),   h = 1/2 psi^2 / ((psi + 1)(2 psi + 1)),   c0 = -1/2 sum_d log((2 psi_d + 1) / (psi_d + 1)^2).
 *   Blocks of 64 x 64 pairs on or above the diagonal, four waves with one 32 x 32 tile each on v_mfma_f32_32x32x2_f32 (the tile below the
 *   diagonal of a diagonal block is not computed), ONE k-ordered chain per output, ascending d; q is walked in panels of 32 through LDS;
 *   g scales the first operand (rounded once per entry); r_i is summed in float64 and rounded once; the epilogue takes
 *   acc - (r_i + r_j) + c0 and writes the one value to [i][j] and [j][i].
 *   Contracts.  Every block of out is EXACTLY symmetric.  A block's bits depend on neither R nor the recording's place in the batch.  A
 *   non-finite entry in row i makes row i and column i of its block NaN; every other entry is BIT-IDENTICAL to the same call with that
 *   row zeroed.  No float atomics: same call, same bits.  R == 0 or a recording with n_r == 0 is a no-op.
 *   SSP_ERR_INVALID before any GPU work: q < 1, g / h / c0 not finite.  SSP_ERR_UNSUPPORTED: q > 1024, a recording with n_r > 4096.
 * ssp_ahc_cluster.  scores: packed as above, not modified; only the entries [i][j] with i < j are read.  Per recording:
 *   Start: the n segments are clusters of size 1, s(i, j) = scores[i][j] for i < j.
 *   lo = n_speakers[r] if n_speakers is given and n_speakers[r] > 0, else max(1, min_clusters);  thr = -inf in the first case, else
 *   threshold.  While the cluster count > lo: take the live pair (a, b), a < b, with the largest s, ties to the smallest a, then the
 *   smallest b; stop unless s(a,b) >= thr; merge b into a (the cluster keeps index a) and for every other live k
 *     linkage 0 (average):  s(a,k) = (fa s(a,k) + fb s(b,k)) / (fa + fb) in fp32, fa = (float)size_a, fb = (float)size_b, every multiply,
 *                           add and divide rounded (no contraction, IEEE division)
 *     linkage 1 (complete): min(s(a,k), s(b,k))          linkage 2 (single): max(s(a,k), s(b,k))
 *   Outputs.  labels_out int32[offsets[R]]: the rank of the segment's cluster among the final clusters ordered by their smallest member;
 *   n_clusters_out int32[R]; merge m of recording r writes (a, b) to row offsets[r] + m of merge_pair_out int32[offsets[R] x 2] and
 *   s(a,b) to merge_score_out float[offsets[R]] (each nullable); unused rows get (-1, -1) and NaN.  n = 0 writes nothing; n = 1 gives
 *   label 0 and count 1.  An n_speakers[r] above n_r simply means no merge.  n_speakers is a HOST array.
 *   Non-finite scores.  A recording with a non-finite entry above its diagonal gets label -1 on all segments, count -1 and every merge
 *   row unused; every other recording is unaffected, bit for bit.
 *   Kernel.  One 256-thread workgroup per recording, the longest first, no communication between workgroups, no spin or claim loops;
 *   every loop has a trip count known on entry (at most n - 1 merges).  The working copy sits in LDS up to n = 192 (row stride n | 1)
 *   and in a workspace the ctx owns above that.  A per-row best (order-preserving key, lowest column) over the live columns j > i sits in
 *   LDS; the arg-max of a merge is one 64-bit integer max over (key << 32 | ~row).  After a merge row a and the rows whose best pointed at
 *   a or b are rescanned, the others compare their one changed entry (an equal entry wins if its column is lower).  -0.0 counts as +0.0.
 *   SSP_ERR_INVALID before any GPU work: linkage not 0..2, a NaN threshold (+-inf are allowed), min_clusters < 1, an n_speakers[r] < 0.
 *   SSP_ERR_UNSUPPORTED: a recording with n_r > 4096.
 * Contracts of both, as ssp_plda_score: device pointers at any 4-byte alignment; with device pointers the calls are stream-ordered and
 *   never wait on the host (once the ctx's tables and workspace have grown to the batch); SSP_HOST stages the inputs and waits for the
 *   results.  An error leaves the ctx usable.  kernel_ms: device time of the kernels, copies excluded (asking for it waits). */
int ssp_pairwise_size(const ssp_segments* seg, int64_t* total_out);
int ssp_pairwise_scores(ssp_ctx* ctx, const float* X, const ssp_segments* seg, int32_t q, const float* g, const float* h, float c0,
                        float* out, int where, float* kernel_ms);
int ssp_ahc_cluster(ssp_ctx* ctx, const float* scores, const ssp_segments* seg, int32_t linkage, float threshold, int32_t min_clusters,
                    const int32_t* n_speakers, int32_t* labels_out, int32_t* n_clusters_out, int32_t* merge_pair_out,
                    float* merge_score_out, int where, float* kernel_ms);

/* ---- VB-HMM resegmentation of diarization labels (VBx, Landini et al. 2022: "Bayesian HMM clustering of x-vector sequences"), for a batch
 *      of recordings: the second pass behind AHC.  It re-assigns windows that greedy merging misplaced, smooths the label sequence in time
 *      and lets superfluous clusters die out.  An EXTENSION and UNPINNED: the yardstick is a float64 restatement (tests/vbhmm_oracle.py),
 *      corroborated by brute-force enumeration and the dense linear-Gaussian formulas.  Added to ABI 4 without a version step. ----
 * Model, per recording.  X (T x q): the projected vectors of the recording's windows in time order (plda.Plda.project: within-speaker
 *   covariance I, between-speaker covariance diag(phi)); phi HOST float[q], >= 0; rho = X sqrt(phi).  S HMM states, 1 <= S <= 64;
 *   recording r uses S_r = clamp(n_init[r], 1, S) live states (S_r = S if n_init is NULL); states >= S_r are inert: pi = gamma = 0
 *   throughout, they add 0 to every sum.
 *   Start: pi_s = 1 / S_r; row t of gamma is the softmax over the live states of init_smoothing * onehot(init_labels[t]); a label
 *   outside [0, S_r) gives the uniform row.
 *   Iteration i = 0, 1, ...:
 *     1. N_s = sum_t gamma_ts                               2. invL_sd = 1 / (1 + (Fa/Fb) N_s phi_d)
 *     3. alpha_sd = (Fa/Fb) invL_sd sum_t gamma_ts rho_td   4. G_t = -1/2 (sum_d x_td^2 + q ln 2 pi)
 *     5. ll_ts = Fa (sum_d rho_td alpha_sd - 1/2 sum_d (invL_sd + alpha_sd^2) phi_d + G_t)
 *     6. forward-backward with initial probabilities pi and transitions tr[i][j] = P delta_ij + (1 - P) pi_j (P = loop_prob): the new
 *        gamma (every row sums to 1) and ln p(X)
 *     7. ELBO_i = ln p(X) + 1/2 Fb sum_{s,d} (ln invL_sd - invL_sd - alpha_sd^2 + 1)
 *     8. pi_s proportional to gamma_0s + sum_{t>=1} xi_t(any -> s by the non-loop branch)
 *          = gamma_0s + (1 - P) pi_s sum_{t>=1} exp(lse_i lfw[t-1][i] + ll_ts + lbw[t][s] - ln p(X)), normalised to sum 1
 *     9. stop after this iteration if i > 0 and ELBO_i - ELBO_{i-1} < epsilon, or if i = max_iters - 1.
 *   The gamma and pi of the last iteration run are the result.
 * Outputs, per recording.  states_out int32[offsets[R]] (nullable): arg max_s gamma_ts, ties to the lowest s.  labels_out
 *   int32[offsets[R]]: the rank of that state among the states that win at least one row, ordered by the smallest row they win (AHC's
 *   label convention).  n_speakers_out int32[R]: the number of such states.  n_iters_out int32[R]: iterations run.  elbo_out
 *   double[R x max_iters] (nullable): NaN beyond n_iters.  gamma_out float[offsets[R] x S], pi_out float[R x S], loglik_out
 *   float[offsets[R] x S]: ll of the last iteration (each nullable).  Inert columns of gamma and pi are 0; inert columns of loglik are
 *   UNSPECIFIED.  A recording without rows writes nothing.  init_labels int32[offsets[R]] and n_init int32[R] sit on the side `where`
 *   names and are read on the device only: ssp_ahc_cluster's labels_out and n_clusters_out feed the call with no read-back.
 *   A recording with a non-finite entry in X gets labels and states -1, n_speakers -1, n_iters 0 and NaN in gamma, pi, loglik and elbo;
 *   every other recording keeps the bits it has without that recording.  R == 0 or T == 0 is a no-op.  No float atomics: same call, same
 *   bits; a recording alone gives the bits it has in a batch (they depend on its T, q, S and numbers only).
 * Kernel.  A row pre-pass (one wave per row) gives G_t, float64 inside, NaN for a row with a non-finite entry.  Then one 256-thread
 *   workgroup per recording, longest first, runs the whole iteration loop: one launch per residency form and call, no host round trip
 *   per iteration, no communication between workgroups, no spin or claim loops; every loop has a trip count known on entry.  S is padded
 *   to SP = 16, 32 or 64 columns (template instances).  The two products of an iteration run on v_mfma_f32_16x16x4_f32 with ONE ascending
 *   k-ordered chain per output: gamma^T rho with a wave per 64 columns of q (k = t), rho alpha^T with a wave per 16 rows (k = d); rho is
 *   formed from X as it is loaded and never stored.  Forward-backward is the O(T S) structured recursion in the per-step-normalised
 *   linear domain, states on the lanes of one wave: forward a_t = b_t o (P a-hat_{t-1} + (1 - P) pi) with b_ts = exp(ll_ts - max ll_t.),
 *   backward beta_t = P y + (1 - P) sum_j pi_j y_j with y = b_{t+1} o beta-hat_{t+1}, gamma_t proportional to a-hat_t o beta-hat_t, the
 *   pi update from the same scaled quantities; ln p(X) = sum_t (ln c_t + max ll_t.), the ELBO and the stop decision are float64.  The
 *   backward pass runs BEHIND the forward pass on the same wave, not beside it: that takes two T x SP buffers, not three.
 *   Residency.  alpha (SP x (q | 1) floats) sits in LDS when it takes at most SSP_VBHMM_ALPHA_LDS_BYTES, else in the ctx's grow-only
 *   workspace; the two T x SP float buffers (ll; a-hat, then gamma) sit in LDS when alpha's LDS share plus 8 T SP bytes is at most
 *   SSP_VBHMM_LDS_BYTES, else in the workspace.
 *   SSP_ERR_INVALID before any GPU work: q < 1, S < 1, max_iters < 1; loop_prob outside [0, 1); Fa or Fb not finite and > 0;
 *   init_smoothing not finite and >= 0; epsilon NaN (+-inf are allowed: -inf never stops early); phi non-finite or negative.
 *   SSP_ERR_UNSUPPORTED: S > 64, q > 1024, max_iters > 100, a recording with more than 4096 rows.
 *   Contracts as ssp_ahc_cluster: device pointers at any 4-byte alignment; with SSP_DEVICE the call is stream-ordered on the ctx's stream
 *   and never waits on the host (once the ctx's tables and workspace have grown to the batch); SSP_HOST goes through the staging scope and
 *   waits for the results.  An error leaves the ctx usable.  kernel_ms: device time of the kernels (asking for it waits). */
#define SSP_VBHMM_LDS_BYTES 155648
#define SSP_VBHMM_ALPHA_LDS_BYTES 65536
int ssp_vbhmm_resegment(ssp_ctx* ctx, const float* X, const ssp_segments* seg, int32_t q, const float* phi, const int32_t* init_labels,
                        const int32_t* n_init, int32_t S, float loop_prob, float Fa, float Fb, float init_smoothing, int32_t max_iters,
                        double epsilon, int32_t* labels_out, int32_t* states_out, int32_t* n_speakers_out, int32_t* n_iters_out,
                        double* elbo_out, float* gamma_out, float* pi_out, float* loglik_out, int where, float* kernel_ms);

/* k-means++ seeding for the k-means start of the same fits (GMM_UBM.py:158-170: GaussianMixture(init_params='kmeans'), sklearn's default;
 * sklearn cluster/_kmeans.py:kmeans_plusplus), for P seeding PROBLEMS (one per model and start) in ONE launch, one workgroup each, with
 * the random numbers handed in.  feats: float[n_rows x D] on the side `where` names (any 4-byte alignment).  Problem p has n_sel[p] rows:
 * sel == NULL: rows [row_off[p], row_off[p] + n_sel[p]) of feats; sel != NULL: the rows sel[row_off[p] .. row_off[p] + n_sel[p]) (HOST
 * int64 row numbers, concatenated, sorted per problem: the subsample the caller drew) — row_off then indexes sel.  Problems may come in
 * any order, leave gaps and overlap.  first[p]: position of the first centre among the problem's rows; u: HOST double[P x (K-1) x L]
 * uniforms in [0, 1), L = 2 + (int)ln K candidates per step.
 * Per problem, in float64 on the float32 rows: d2[i] = |x_i - x_first|^2; then for k = 1 .. K-1: cum = inclusive prefix sum of d2,
 * total = cum[n-1]; cand[l] = min(n-1, #{i : cum[i] < u[k-1][l] * total}) (numpy searchsorted, side='left', and the clip);
 * dc[i][l] = |x_i - x_cand[l]|^2; pot[l] = sum_i min(d2[i], dc[i][l]); the pick is cand[b], b the FIRST arg-min of pot;
 * d2[i] = min(d2[i], dc[i][b]).  All rows equal (total == 0): every candidate is position 0, no error.
 * Outputs (HOST): seed_rows_out int64[P x K]: the picks as absolute row numbers of feats; centres_out double[P x K x D]: those rows
 * widened (NULL: not wanted).  Every sum has a fixed shape (no floating-point atomics): the same call gives the same bits every time,
 * and a problem's picks do not depend on the other problems of the launch.
 * SSP_ERR_INVALID, each found before any GPU work: P < 1, K < 1, a problem with n_sel < 1, a row outside [0, n_rows), first outside
 * [0, n_sel), a u outside [0, 1) (the messages name the problem).  SSP_ERR_INVALID after the launch: a problem whose total is not finite
 * (a NaN or infinite row; K >= 2) — the message names the first such problem, no output is written, and nothing stays behind in the ctx.
 * SSP_ERR_UNSUPPORTED: D > 64 (a wave stages 64 rows through LDS), more than 24 candidates per step, a problem of 2^31 rows.
 * Design point: n_sel <= ~32 k rows per problem (the subsample cap max(20000, 50 K)); larger problems are correct, still on one workgroup.
 * Work: one upload of the draws / lists, one launch, one result copy + host wait. */
int ssp_kmeanspp_seed(ssp_ctx* ctx, int32_t P, int32_t K, int32_t D, const float* feats, int64_t n_rows, int where,
                      const int64_t* row_off, const int64_t* n_sel, const int64_t* sel, const int64_t* first, const double* u,
                      int64_t* seed_rows_out, double* centres_out, float* kernel_ms);

/* ---- DTW template matching: replaces the distance_dtw double loop of MFCC_DTW.py:57-108,187-217
 *      (dtw.accelerated_dtw(x, y, dist='euclidean'), warp 1) for every (query, template) pair ---- */
/* xq: float[total query rows x dim] with q_seg row offsets; xt, t_seg likewise for the templates (dim = 1: the reference's
 * flattened _MFCC sequences).  dist_out: float[n_q x n_t] = D1[r-1][c-1]; normalize != 0 divides by (r + c) (dtw <= 1.3.3).
 * Empty sequences: a pair whose query or template has no row (or both) scores +inf, with normalize too (the package would fail); the
 * other pairs of the call are not affected.
 * Non-finite input: a pair scores what the float64 recurrence with NaN-propagating minima (numpy's np.minimum) gives, wherever in the
 * sequence the bad element sits: NaN if either sequence holds a NaN, or both hold the same infinity in the same coordinate (inf - inf);
 * otherwise +inf if either holds an infinity; pairs of finite sequences keep their bits.  normalize does not change a NaN or +inf.
 * (The dtw package's own Python min() depends on the order of its operands when one is NaN; it is not followed.)
 * Finite input: float32 arithmetic, |dist - float64| <= 1.01 (r + c + k) 2^-24 dist with k = 1 at dim 1 and dim + 3 above. */
int ssp_dtw_distances(ssp_ctx* ctx, const float* xq, const ssp_segments* q_seg, const float* xt, const ssp_segments* t_seg,
                      int32_t dim, int32_t normalize, float* dist_out, int where, float* kernel_ms);

/* The dtw_method = 2 branch of the same matcher (MFCC_DTW.py:69-70: fastdtw(x, y, dist=euclidean), radius 1): the FastDTW approximation
 * for every (query, template) pair of 1-D sequences, float64 like the package.  Host arrays in, dist_out: HOST double[n_q x n_t]. */
int ssp_fastdtw_distances(ssp_ctx* ctx, const float* xq, const ssp_segments* q_seg, const float* xt, const ssp_segments* t_seg,
                          int32_t radius, double* dist_out, float* kernel_ms);

/* One pair WITH the warping path — what generate_template (MFCC_DTW.py:187-217) takes from accelerated_dtw: d and
 * path = _traceback(D0) (first minimum of diagonal / up / left at every step), computed in float64 like the package.
 * x: HOST float[r x dim], y: HOST float[c x dim]; path_i_out / path_j_out: HOST int32[r + c] (path_len_out entries are written). */
int ssp_dtw_path(ssp_ctx* ctx, const float* x, int64_t r, const float* y, int64_t c, int32_t dim, double* dist_out,
                 int32_t* path_i_out, int32_t* path_j_out, int32_t* path_len_out);

/* Every speaker's template in batched launches — the generate_template loop of load_train (MFCC_DTW.py:122-152, 187-217).
 * x: HOST double[seq_off[n_seq] x dim], the sequences' rows back to back (seq_off: HOST int64[n_seq + 1], from 0, increasing); group g
 * owns the sequences grp_off[g] .. grp_off[g + 1] - 1 (HOST int64[n_grp + 1], from 0 to n_seq, increasing).  A group's template is its
 * first longest sequence, updated with the group's other sequences in index order: warp the sequence onto the template (the
 * accelerated_dtw path), average the aligned values, keep the first path entry of every template index.  Round k of all groups is one
 * launch of a forward kernel (float64 wavefront that stores one direction byte per cell instead of D1) and one of a traceback-and-update
 * kernel; all rounds are enqueued on the context's stream without a host wait and the call returns after one.  As in ssp_dtw_path (which
 * api.dtw_path feeds float32 arrays) the cost of a cell is taken from operands ROUNDED TO float32, accumulated in float64: a deviation
 * of the existing single-pair path from the reference that is kept here, not changed, so that both give the same bits.
 * tmpl_out: HOST double[sum of the groups' longest lengths x dim], templates back to back; tmpl_off_out: HOST int64[n_grp + 1], their
 * row offsets.  A group of one sequence returns that sequence.  workspace_bytes caps the direction store of one round (0 = 1 GiB):
 * consecutive groups share launches while they fit, a pair that exceeds the cap alone raises it to its need (rows x columns padded to
 * a multiple of 4 bytes); the result does not depend on the cap.  Five device allocations per call, whatever the number of pairs.
 * SSP_ERR_INVALID: null pointers, dim < 1, no group, an empty group or sequence, offsets that do not increase, a non-finite value in x
 * (scanned before the first launch).  SSP_ERR_UNSUPPORTED: a pair beyond ssp_dtw_path's limits (r or c > 2^20, r x c > 5e8). */
int ssp_dtw_templates(ssp_ctx* ctx, const double* x, const int64_t* seq_off, int64_t n_seq, const int64_t* grp_off, int64_t n_grp,
                      int32_t dim, int64_t workspace_bytes, double* tmpl_out, int64_t* tmpl_off_out, float* kernel_ms);

/* ---- d-vector network forward: one Dense layer Y = act(X W + b) of the speaker network the reference runs with
 *      spkModel.predict (d_vector.py:171-189 builds Dense(256) x 4 with ReLU between; predict at d_vector.py:298-299,327,348) ---- */
/* X: float[N x d_in]; Wt: float[units x d_in] = the Keras kernel (d_in x units) TRANSPOSED; bias: float[units] (nullable);
 * relu != 0 applies max(0, .); Y: float[N x units].  All four arrays live on the side `where` names.
 * Non-finite input.  A NaN stays a NaN through ReLU (numpy's maximum, Keras; not C's fmaxf): Y[n][u] is NaN, +inf or -inf exactly
 * where the float64 evaluation of the same float32 operands is, so a NaN anywhere in sample n makes row n NaN, and +-inf propagates
 * by IEEE arithmetic (inf - inf and 0 * inf are NaN).  No other sample's row moves by a bit.
 * A sample's output bits do not depend on the batch it is in (N, its position, its neighbours).
 * Error against float64: |Y - ref| <= 1.01 (d_in + 1) 2^-23 (sum_k |x_k| |w_ku| + |b_u|) per element (tests/dense_cases.py). */
int ssp_dense_forward(ssp_ctx* ctx, const float* X, int64_t N, int32_t d_in, const float* Wt, const float* bias,
                      int32_t units, int32_t relu, float* Y, int where, float* kernel_ms);

/* The whole network as one object: n_layers Dense layers, layer l = (Wt[l]: HOST float[dims[l+1] x dims[l]] = Keras kernel transposed,
 * bias[l]: HOST float[dims[l+1]] or NULL, relu[l]).  ssp_dnn_forward = spkModel.predict: X float[N x dims[0]] -> Y float[N x dims[n_layers]].
 * Layers whose input and output widths are <= 256 (the reference's three hidden-to-hidden / output layers) run inside one kernel with
 * the activations kept in registers between layers; wider layers in front of them (the 1274-input layer) run one GEMM launch each.
 * Non-finite input: ssp_dense_forward's rule, layer by layer.  A NaN passes every ReLU; +-inf reaches the output as the float64
 * evaluation carries it.  The zero padding of a layer narrower than 256 takes no part: a padded unit leaves its layer as exactly 0
 * whatever the sample holds (never 0 * inf = NaN).  A sample's output bits do not depend on the batch it is in. */
int ssp_dnn_create(ssp_ctx* ctx, int32_t n_layers, const int32_t* dims, const float* const* Wt, const float* const* bias,
                   const int32_t* relu, ssp_dnn** out);
int ssp_dnn_destroy(ssp_dnn* dnn);
int ssp_dnn_forward(ssp_dnn* dnn, const float* X, int64_t N, float* Y, int where, float* kernel_ms);

/* ---- d-vector recurrent network forward: the LSTM(128) whose last hidden state is the embedding (d_vector.py:271-294 inference_lstm;
 *      spkModel.predict with the default model_name 'lstm' at d_vector.py:297-299, 330-331, 347-348).  Keras' cell, return_sequences
 *      False, zero initial state, no mask; gate blocks in the order i | f | c | o:
 *        z = x_t W + h_{t-1} U + b;  i = s(z_i), f = s(z_f), g = tanh(z_c), o = s(z_o);  c_t = f c_{t-1} + i g;  h_t = o tanh(c_t)
 *      recurrent_activation names s: 0 hard_sigmoid = clip(0.2 z + 0.5, 0, 1) (stand-alone Keras <= 2.2's default) | 1 logistic sigmoid
 *      (Keras >= 2.3, tf.keras).  The caller chooses; there is no default. ---- */
/* W: HOST float[d_in x 4 units], U: HOST float[units x 4 units], bias: HOST float[4 units] or NULL — layer.get_weights() as it is.
 * units: a multiple of 16 up to 128; d_in up to 64; anything else answers SSP_ERR_UNSUPPORTED (no other path exists). */
int ssp_lstm_create(ssp_ctx* ctx, int32_t d_in, int32_t units, const float* W, const float* U, const float* bias,
                    int32_t recurrent_activation, ssp_lstm** out);
int ssp_lstm_destroy(ssp_lstm* lstm);
/* feats: float[total frames x d_in] row-major laid out by frame_seg — what ssp_mfcc_run writes; sequence s is rows
 * [offsets[s], offsets[s + 1]) and runs for its own length (a sequence without frames gives the zero vector).  h_out: float[n_seq x units]
 * = h_T of every sequence.  A sequence's output bits do not depend on the batch it is in.  One kernel: 16 sequences per wave on exact
 * fp32 MFMA, h and c in registers for the whole sequence, the weights streamed per time step through LDS. */
int ssp_lstm_forward(ssp_lstm* lstm, const float* feats, const ssp_segments* frame_seg, float* h_out, int where, float* kernel_ms);
/* The operand-order image ssp_lstm_create uploads, built on the host (no device, no ctx).  With HT = 1, 2, 4 or 8 tiles of 16 hidden
 * units covering `units`, dT = ceil(d_in / 16) and G = dT + HT input groups of 16:
 *   image[(((j G + g) 4 + q) 64 + lane) 4 + r] = row k, column q units + u of W (g < dT: k = 16 g + 4 (lane >> 4) + r) or of U
 *   (g >= dT: k = 16 (g - dT) + 4 (lane >> 4) + r), u = 16 j + (lane & 15); zero where k or u lies beyond the matrix;
 *   then bias as [4 gates][16 HT], zero padded.
 * n_floats_out (nullable) receives the image's length, HT G 1024 + 64 HT; image_out == NULL only asks for that length. */
int ssp_lstm_pack_weights(int32_t d_in, int32_t units, const float* W, const float* U, const float* bias, float* image_out,
                          int64_t* n_floats_out);

/* ---- d-vector conv + GRU network forward (since without a version step, like the LSTM entries): the pieces of inference_gru
 *      (d_vector.py:213-269) — Conv2D(64, 5x5, strides 2, padding 'same') :216-221, TimeDistributed(Flatten) :226, 3 x GRU(1024,
 *      return_sequences=True) :229-231, the mean over time :234-237, Dense(512) :240 (ssp_dense_forward) and K.l2_normalize :243-246 — the
 *      network d_vector.py:389 evaluates as model_name 'lstm_conv'.  Unpinned: the reference tree holds no GRU weights or outputs.
 *      One GRU layer, Keras' cell at inference, gate blocks z | r | h, zero initial state, return_sequences:
 *        reset_after 0 (stand-alone Keras), bias [3 units] or NULL:
 *          z = s(x W_z + b_z + h U_z);  r = s(x W_r + b_r + h U_r);  hh = tanh(x W_h + b_h + (r . h) U_h)
 *        reset_after 1 (tf.keras 2), bias [2 x 3 units] = input row, recurrent row, or NULL:
 *          z = s(x W_z + b_iz + h U_z + b_rz);  r likewise;  hh = tanh(x W_h + b_ih + r . (h U_h + b_rh))
 *        h_t = z . h_{t-1} + (1 - z) . hh
 *      recurrent_activation names s: 0 hard_sigmoid = clip(0.2 z + 0.5, 0, 1) | 1 logistic sigmoid.  The weights file records neither
 *      switch: the caller names both, there is no default. ---- */
/* W: HOST float[d_in x 3 units], U: HOST float[units x 3 units], bias as above — layer.get_weights() as it is.  units: a multiple of
 * 16 up to 1024; d_in up to 4096; anything else answers SSP_ERR_UNSUPPORTED, a bad switch or a null kernel SSP_ERR_INVALID, both
 * before any GPU work. */
int ssp_gru_create(ssp_ctx* ctx, int32_t d_in, int32_t units, const float* W, const float* U, const float* bias,
                   int32_t recurrent_activation, int32_t reset_after, ssp_gru** out);
int ssp_gru_destroy(ssp_gru* gru);
/* X: float[N x T x d_in]; seq_out (nullable): float[N x T x units] = h_t of every step; mean_out (nullable): float[N x units] = the mean
 * of h_t over t, summed with t ascending (d_vector.py:234-237).  The input projection of all rows is one GEMM, the recurrence one launch
 * per time step (two with reset_after 0) of an exact-fp32 MFMA GEMM against the packed U with the gate arithmetic in its epilogue, on
 * the ctx stream.  A large batch runs in slabs of whole chunks under the workspace cap (projection buffer, kept on the ctx and shared
 * by the layers of a network; the output sequence when seq_out is NULL, on the host or not 16-byte aligned; z and r . h with
 * reset_after 0); one chunk always runs.  A chunk's output bits do not depend on N, on the slab size or on its place in the batch. */
int ssp_gru_forward(ssp_gru* gru, const float* X, int64_t N, int32_t T, float* seq_out, float* mean_out, int where, float* kernel_ms);
/* the workspace cap of one forward call in bytes (default 2 GiB) and the chunks per slab the last call used */
int ssp_gru_set_workspace(ssp_gru* gru, size_t bytes);
int ssp_gru_last_slab(const ssp_gru* gru, int64_t* chunks_out);
/* Conv2D with one input channel, channels last, linear activation, TensorFlow's `same` padding (d_vector.py:216-221): out = ceil(in / s),
 * pad = max((out - 1) s + k - in, 0), pad / 2 in front and the rest behind; a cross-correlation.  X: float[N x T x D]; K: float[kh x kw x 1 x F]
 * (the Keras kernel as it is); bias: float[F] (nullable); Y: float[N x To x Do F], element (f_out F + c) of a time step — the
 * TimeDistributed(Flatten) of d_vector.py:226 is this layout.  kh, kw up to 7, F up to 256, strides 1 or 2 (SSP_ERR_UNSUPPORTED beyond).
 * All arrays live on the side `where` names. */
int ssp_conv2d_same_forward(ssp_ctx* ctx, const float* X, int64_t N, int32_t T, int32_t D, const float* K, const float* bias, int32_t kh,
                            int32_t kw, int32_t F, int32_t sh, int32_t sw, float* Y, int where, float* kernel_ms);
/* K.l2_normalize(x, axis=1) (d_vector.py:243-246): Y = X / sqrt(max(sum_k X_k^2, eps)) per row (Keras' eps: 1e-12; an all-zero row stays
 * zero).  X, Y: float[N x d]; Y may be X. */
int ssp_l2_normalize(ssp_ctx* ctx, const float* X, int64_t N, int32_t d, float eps, float* Y, int where, float* kernel_ms);

/* ---- x-vector extractor forward (since without a version step, like the LSTM and GRU entries): the time-delay network of Snyder et
 *      al. 2018 ("X-vectors: robust DNN embeddings for speaker recognition") — frame layers, statistics pooling, segment layers — that
 *      Kaldi's nnet3 recipes, VBx, SpeechBrain and wespeaker put between the features and the back ends above (ssp_plda_*, ssp_snorm_*,
 *      ssp_pairwise_scores / ssp_ahc_cluster, ssp_vbhmm_resegment).  An EXTENSION and UNPINNED: the reference has no TDNN and none of
 *      those toolkits or their models is at hand; the forms below are recalled from them, tests/xvector_oracle.py restates them in
 *      float64 and tests/test_xvector_host.py corroborates the restatement against torch.nn.functional.conv1d in float64.  Inference only.
 *        Frame layer    T rows of width d_in -> T - (taps - 1) dil rows of width units ("valid": no padding, the sequence shrinks):
 *                         z[t][u] = b[u] + sum_{j < taps} sum_{c < d_in} x[t + j dil][c] W[u][j][c]
 *                         y[t][u] = scale[u] act(z[t][u]) + offset[u]      act = max(0, .) if relu else the identity
 *                       scale / offset are nullable (1 / 0) and applied as ONE fused multiply-add.  Kaldi's affine -> ReLU -> batch-norm
 *                       (no learnt scale) and SpeechBrain's conv -> ReLU -> BN are this form with the inference-time BN in scale /
 *                       offset; conv -> BN -> ReLU folds into W and b.  A NaN stays a NaN through the ReLU (ssp_dense_forward's rule).
 *        Network        n_f frame layers; statistics pooling over the rows of the last one; n_s >= 0 segment layers of the same form
 *                       with taps = 1 on the pooled vector.  The output is the last segment layer given (for Kaldi's embedding: the
 *                       layers up to segment6 with relu = 0), the pooled vector itself with n_s = 0.  R = 1 + sum (taps - 1) dil is
 *                       the receptive field: a sequence of T frames has T - R + 1 pooled rows.  The standard network: (taps, dil) =
 *                       (5,1), (3,2), (3,3), (1,1), (1,1), widths 512, 512, 512, 512, 1500, pooled width 3000, a 3000 -> 512 segment
 *                       layer, R = 15.
 *        Pooling        of rows t in [a, b), n = b - a, of width C gives 2 C values, the means then the deviations:
 *                         mean_c = sum_t x[t][c] / n;   dev_c = sqrt(max(sum_t (x[t][c] - mean_c)^2 / n, var_floor))
 *                       — the population variance in the CENTRED form, accumulated in float64 with t ascending (two passes), rounded to
 *                       float32 once.  A column constant over the window gives exactly sqrt(var_floor).  n = 0 (a sequence or window
 *                       of fewer than R frames) gives a row of NaN — numpy's mean of nothing — and the call still answers SSP_OK; no
 *                       other row moves by a bit.
 *        Pool windows   pool_win: HOST int64[n_win x 3] of (sequence, first, end) in INPUT frame coordinates inside the sequence,
 *                       sequences non-decreasing, 0 <= first <= end <= T_sequence (else SSP_ERR_INVALID before any GPU work); window w
 *                       gives output row w.  The embedding of a window is DEFINED as the embedding of frames [first, end) extracted
 *                       as a sequence of their own — the pooling of the last frame layer's rows [first, end - R + 1) of the sequence
 *                       — and has the same BITS as that stand-alone extraction: the frame layers run once per sequence, only the
 *                       pooling and the segment layers run per window.  NULL: one window per sequence, covering all of it.
 *        Non-finite     the output is non-finite exactly where the float64 evaluation of the same float32 operands is: a NaN in frame
 *                       t reaches exactly the pooled rows whose receptive field covers t and makes every column NaN in exactly the
 *                       embeddings that pool such a row; every other sequence's and window's row keeps its bits.
 *      A sequence's (window's) output bits depend neither on the batch it is in nor on the slab it lands in.
 *      Limits (SSP_ERR_UNSUPPORTED before any GPU work): d_in and units of a frame layer up to 8192, taps up to 16, (taps - 1) dil up
 *      to 1024, up to 64 frame and 64 segment layers, pooled width and segment widths up to 2^21. ---- */
/* ONE frame layer.  X: float[frames x d_in] laid out by frame_seg (what ssp_mfcc_run and ssp_featnorm_sliding write); W:
 * float[units x taps x d_in]; bias, scale, offset: float[units] (nullable); all on the side `where` names, any 4-byte alignment.
 * Y: float[frames x units] with the ROW INDEX of X: output t of sequence s stands at row offsets[s] + t, left-aligned in the sequence;
 * out_len (HOST int64[n_seq], nullable) receives the valid lengths max(0, T_s - (taps - 1) dil).  The last (taps - 1) dil rows of each
 * sequence in Y are written but UNSPECIFIED (they hold sums that run into the next sequence or past the end, where the input reads as
 * zero); rows in front of offsets[0] are neither read nor written.  Feeding Y and frame_seg to the next layer is therefore correct as
 * it stands: a valid row never reads an unspecified one.  One launch of an implicit-im2col GEMM on the exact-fp32 MFMA: one k-ordered
 * chain per output, taps ascending, channels ascending.
 * Error against float64, before scale / offset: |z - ref| <= 1.01 (K + 1) 2^-23 (sum |x| |w| + |b|), K = taps d_in; with them multiply
 * by |scale| and add 2^-23 |y| (tests/test_xvector_gpu.py). */
int ssp_tdnn_forward(ssp_ctx* ctx, const float* X, const ssp_segments* frame_seg, int32_t d_in, const float* W, const float* bias, int32_t taps,
                     int32_t dilation, int32_t units, int32_t relu, const float* scale, const float* offset, float* Y, int64_t* out_len, int where,
                     float* kernel_ms);
/* The pooling alone.  X: float[frames x dim] laid out by frame_seg; pool_win: HOST int64[n_win x 3] of (sequence, first, end) in X's
 * frame coordinates inside the sequence — rows [first, end) are pooled as they stand, no receptive field is taken off — or NULL: every
 * sequence whole (n_win is then ignored).  out: float[n_win or n_seq x 2 dim].  One workgroup per (window, 256 columns). */
int ssp_stats_pool(ssp_ctx* ctx, const float* X, const ssp_segments* frame_seg, int32_t dim, const int64_t* pool_win, int64_t n_win, double var_floor,
                   float* out, int where, float* kernel_ms);
/* The network as one object.  Everything is a HOST array: units, taps, dilation, relu: int32[n_frame_layers]; W[l]:
 * float[units[l] x taps[l] x d_in_l] (d_in_0 = d_in, d_in_l = units[l - 1]); bias, scale, offset: arrays of pointers to float[units[l]],
 * each array and each entry nullable.  The segment layers likewise with taps = 1: seg_W[l]: float[seg_units[l] x d_in_l], d_in_0 =
 * 2 units[n_frame_layers - 1].  n_frame_layers >= 1, n_segment_layers >= 0. */
int ssp_xvector_create(ssp_ctx* ctx, int32_t d_in, int32_t n_frame_layers, const int32_t* units, const int32_t* taps, const int32_t* dilation,
                       const float* const* W, const float* const* bias, const int32_t* relu, const float* const* scale, const float* const* offset,
                       int32_t n_segment_layers, const int32_t* seg_units, const float* const* seg_W, const float* const* seg_bias,
                       const int32_t* seg_relu, const float* const* seg_scale, const float* const* seg_offset, double var_floor, ssp_xvector** out);
int ssp_xvector_destroy(ssp_xvector* xv);
/* the receptive field R, the pooled width and the embedding width (each nullable) */
int ssp_xvector_info(const ssp_xvector* xv, int32_t* receptive_field, int32_t* pooled_width, int32_t* embed_width);
/* the workspace cap of one forward call in bytes (default 2 GiB): two ping-pong activation buffers of (slab rows x widest frame layer)
 * floats, grow-only and kept on the object; a batch above it runs in slabs of WHOLE sequences, one sequence always runs.
 * ssp_xvector_last_slab: the sequences in the largest slab of the last forward call. */
int ssp_xvector_set_workspace(ssp_xvector* xv, size_t bytes);
int ssp_xvector_last_slab(const ssp_xvector* xv, int64_t* sequences_out);
/* feats: float[total frames x d_in] laid out by frame_seg, which must start at frame 0; pool_win (HOST, nullable) and n_win as above;
 * emb_out: float[n_win or n_seq x embed width].  Ordered on the context's stream: with device pointers the call returns without a host
 * wait once its buffers have grown.  Frame layers: one ssp_tdnn_forward launch each per slab; pooling: one launch; segment layers:
 * ssp_dense_forward, then scale / offset in a launch of their own where given. */
int ssp_xvector_forward(ssp_xvector* xv, const float* feats, const ssp_segments* frame_seg, const int64_t* pool_win, int64_t n_win, float* emb_out,
                        int where, float* kernel_ms);

/* ---- d-vector network training (since without a version step, like the LSTM and GRU entries): nn_model.inference, d_vector.py:168-206 —
 *      the Sequential of Dense / ReLU / Dropout layers :171-194, categorical cross-entropy and Adam(lr=1e-4) :198-203, spk.fit(batch_size
 *      128, epochs 50, shuffled) :205-206.  ReduceLROnPlateau :200, CSVLogger :201 and spkModel.save :210 stay with the host side
 *      (d_vector.nn_model.inference).  Unpinned: the reference tree holds no weights, logs or outputs of this network and Keras is not a
 *      dependency; the arithmetic below is restated from Keras 2's sources and corroborated against torch.autograd only.  All fp32, the
 *      products on the exact-fp32 MFMA; no floating-point atomics: the same seed, data and order give the same bits.
 *        Dense    layer l: y = act(x W_l + b_l), W_l in Keras' (d_in, units) layout; the caller initialises (Keras' Dense defaults are
 *                 glorot_uniform kernels and zero biases; d_vector.nn_model.inference draws them from a seeded numpy generator).
 *        Dropout  after layer l's activation, inverted as in Keras: a kept unit is scaled by 1 / (1 - rate), the others are zero, rate 0
 *                 is the identity.  The decision is counter-based and stateless — a pure function of (seed, step, layer, row inside the
 *                 batch, column), step = the number of steps the trainer had taken before this one:
 *                   mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16           (32-bit, wrapping)
 *                   key = mix(mix(mix(mix(mix(0x9e3779b9 ^ seed_lo) ^ seed_hi) ^ step_lo) ^ step_hi) ^ layer)
 *                   keep(row, col) = (mix(key ^ (row * 4096 + col)) >> 8) >= floor(rate * 2^24)
 *                 It is recomputed in the backward pass, never stored.
 *        Loss     softmax and cross-entropy together on the logits: row maximum subtracted, log-sum-exp.  Keras' clipping of the
 *                 probabilities to [1e-7, 1 - 1e-7] is NOT reproduced (it only matters when a probability underflows 1e-7).  The
 *                 gradient at the logits is (softmax - onehot) / B with B the actual size of that batch: the last batch of an epoch has
 *                 N % batch_size rows, as Keras runs it.  Accuracy counts rows whose arg-max (first index on ties) is the label.
 *        Adam     Keras 2's form, beta1 0.9, beta2 0.999, eps 1e-7 (K.epsilon()) OUTSIDE the root, t counted from 1 over the whole fit:
 *                   m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  lr_t = lr sqrt(1 - b2^t) / (1 - b1^t);  p -= lr_t m / (sqrt(v) + eps)
 *                 (not torch's placement of eps).  One launch over all parameters: they, the gradients, m and v are one flat buffer each. ---- */
/* dims: HOST int32[n_layers + 1]; relu[l] != 0: ReLU after layer l; dropout_rate[l] in [0, 1): dropout after layer l's activation;
 * W[l]: HOST float[dims[l] x dims[l + 1]]; bias: NULL, or bias[l]: HOST float[dims[l + 1]] or NULL (a layer without bias).  The last
 * width is n_class (>= 2).  Widths up to 4096 and max_batch up to 1024, else SSP_ERR_UNSUPPORTED; a null kernel or a rate outside [0, 1)
 * answers SSP_ERR_INVALID; both before any GPU work. */
int ssp_dnn_trainer_create(ssp_ctx* ctx, int32_t n_layers, const int32_t* dims, const int32_t* relu, const float* dropout_rate,
                           const float* const* W, const float* const* bias, int32_t max_batch, ssp_dnn_trainer** out);
int ssp_dnn_trainer_destroy(ssp_dnn_trainer* trainer);
/* One pass of spk.fit over the data (d_vector.py:205-206): ceil(N / batch_size) steps of forward with dropout, loss, backward and Adam at
 * learning rate lr.  X: float[N x dims[0]], labels: int32[N], on the side `where` names; order: HOST int64[N] (step s takes rows
 * order[s batch_size ..]) or NULL for 0..N-1.  The steps are queued on the ctx stream without a host wait; every step leaves its loss
 * sum and its count of correct rows in a slot of a device array, which is read back ONCE at the end and added on the host in float64 in
 * step order: loss_sum = sum over rows of the loss as the steps ran (dropout on, weights moving), n_correct likewise (both nullable).
 * The step counter t continues across calls: an epoch equals its steps issued one batch per call, bit for bit.  SSP_ERR_INVALID before
 * any GPU work: batch_size outside [1, max_batch], an order entry outside [0, N), a label outside [0, n_class) in a HOST array (on the
 * device a label out of range is not read as an index: its row counts as wrong and its loss is the log-sum-exp of its logits).
 * t advances with every step queued: a call that fails half way leaves t in step with the weights it has moved. */
int ssp_dnn_trainer_epoch(ssp_dnn_trainer* trainer, const float* X, const int32_t* labels, int64_t N, const int64_t* order, int32_t batch_size,
                          float lr, uint64_t seed, double* loss_sum, int64_t* n_correct, int where, float* kernel_ms);
/* the validation pass of spk.fit (d_vector.py:205): dropout off, nothing updated (weights, gradients, m, v and t keep their values) */
int ssp_dnn_trainer_evaluate(ssp_dnn_trainer* trainer, const float* X, const int32_t* labels, int64_t N, double* loss_sum, int64_t* n_correct,
                             int where, float* kernel_ms);
/* layer's kernel (dims[l] x dims[l + 1]) or bias (dims[l + 1]) of: the parameters, the LAST step's gradients, Adam's m and v.
 * out: HOST.  Waits for the ctx stream.  A bias of a layer created without one answers SSP_ERR_INVALID. */
enum { SSP_DNN_W = 0, SSP_DNN_B = 1, SSP_DNN_DW = 2, SSP_DNN_DB = 3, SSP_DNN_M_W = 4, SSP_DNN_M_B = 5, SSP_DNN_V_W = 6, SSP_DNN_V_B = 7 };
int ssp_dnn_trainer_read(ssp_dnn_trainer* trainer, int32_t what, int32_t layer, float* out);
int ssp_dnn_trainer_steps(const ssp_dnn_trainer* trainer, int64_t* t); /* steps taken so far (Adam's t) */
/* the dropout generator itself, on the host (no device, no ctx; like ssp_lstm_pack_weights): keep_out HOST uint8[rows x width] = 1 where
 * the unit is kept.  rows up to 1024, width up to 4096. */
int ssp_dropout_keep(uint64_t seed, int64_t step, int32_t layer, int32_t rows, int32_t width, float rate, uint8_t* keep_out);

/* ---- recurrent d-vector network training (since without a version step, like the entries above): nn_model.inference_lstm,
 *      d_vector.py:271-294 — LSTM(128) over the (T, d_in) chunk :274, Dense(n_class) softmax on the last hidden state :278, categorical
 *      cross-entropy and Adam(lr=1e-4) :281-284, spk.fit(batch_size 128, epochs 50, shuffled) :289-290.  ReduceLROnPlateau :286, CSVLogger
 *      :287 and spkModel.save :294 stay with the host side (d_vector.nn_model.inference_lstm).  Unpinned: the reference tree holds no
 *      weights, logs or outputs of this network and Keras is not a dependency; the arithmetic is restated and corroborated against
 *      torch.autograd only.  All fp32, the products on the exact-fp32 MFMA.
 *        Network  one LSTM(units) over a fixed-length chunk; Keras' cell exactly as stated for ssp_lstm_forward above (gate blocks
 *                 i | f | c | o, zero initial state, no mask; recurrent_activation 0 hard_sigmoid | 1 sigmoid); the last hidden state
 *                 feeds Dense(n_class) and a softmax.  No dropout, no recurrent dropout, no gradient clipping.
 *        Loss, accuracy, Adam: the dense trainer's, in the words of the section above — softmax and cross-entropy together on the
 *                 logits, the gradient at the logits (softmax - onehot) / B with B the actual batch (the tail batch included), Keras 2's
 *                 Adam with eps 1e-7 outside the root and t counted over the whole fit, one Adam launch over flat parameter, gradient, m
 *                 and v buffers (W | U | b | Wd | bd).
 *        Backward through time, for t = T-1 .. 0, dh starting as dlogits Wd^T and dc at 0:
 *                   do = dh tanh(c_t);  dc += dh o (1 - tanh^2(c_t))
 *                   dz = [dc g s'(i) | dc c_{t-1} s'(f) | dc i (1 - g^2) | do s'(o)]
 *                   dW += x_t^T dz;  dU += h_{t-1}^T dz;  db += sum over rows of dz;  dh = dz U^T;  dc = dc f
 *                 sigmoid: s'(s) = s (1 - s).  hard_sigmoid: s' = 0.2 where the fp32 activation lies strictly inside (0, 1) and 0
 *                 elsewhere (Keras' clip passes no gradient at or beyond the bounds).
 *        Determinism: no floating-point atomic anywhere.  A sequence is one MFMA column in both recurrent kernels; the sums over the
 *                 B T rows in dW / dU / db, the split of K over waves and the loss have a fixed partition and a fixed order: the same
 *                 seed, data and order give the same bits.
 *      The forward kernel gives a workgroup 16 sequences and each of its units / 16 waves one hidden tile whose slice of [W; U] stays in
 *      registers over the T steps, x_t and h_{t-1} in LDS, one barrier per step; it stashes x_t, h_t, c_t and the gate activations per
 *      (row, t) in a workspace allocated at create (T max_batch (d_in + 6 units) floats).  The backward kernel runs the same
 *      decomposition in reverse and leaves dz in the stash; the weight gradients are GEMMs over it. ---- */
/* W: HOST float[d_in x 4 units], U: HOST float[units x 4 units], bias: HOST float[4 units] or NULL (Keras layout, as ssp_lstm_create);
 * Wd: HOST float[units x n_class], bd: HOST float[n_class] or NULL.  units: a multiple of 16 up to 128, d_in up to 64 (as for the forward
 * pass), T in [1, 1024], n_class in [2, 4096], max_batch in [1, 1024], else SSP_ERR_UNSUPPORTED; a null W / U / Wd or a bad activation
 * code answers SSP_ERR_INVALID; both before any GPU work. */
typedef struct ssp_lstm_trainer ssp_lstm_trainer;
int ssp_lstm_trainer_create(ssp_ctx* ctx, int32_t d_in, int32_t units, int32_t n_class, int32_t T, int32_t recurrent_activation, const float* W,
                            const float* U, const float* bias, const float* Wd, const float* bd, int32_t max_batch, ssp_lstm_trainer** out);
int ssp_lstm_trainer_destroy(ssp_lstm_trainer* trainer);
/* One pass of spk.fit over the data (d_vector.py:289-290): ceil(N / batch_size) steps of forward, loss, backward and Adam at learning rate
 * lr.  X: float[N x T x d_in], labels: int32[N], on the side `where` names; order: HOST int64[N] (step s takes rows order[s batch_size ..],
 * gathered inside the kernel's loads) or NULL for 0..N-1.  The steps are queued on the ctx stream without a host wait; every step leaves
 * its loss sum and its count of correct rows in a slot of a device array, which is read back ONCE at the end and added on the host in
 * float64 in step order (both nullable).  The step counter t continues across calls: an epoch equals its steps issued one batch per call,
 * bit for bit.  SSP_ERR_INVALID before any GPU work: batch_size outside [1, max_batch], an order entry outside [0, N), a label outside
 * [0, n_class) in a HOST array (on the device a label out of range is not read as an index: its row counts as wrong and its loss is the
 * log-sum-exp of its logits).  t advances with every step queued. */
int ssp_lstm_trainer_epoch(ssp_lstm_trainer* trainer, const float* X, const int32_t* labels, int64_t N, const int64_t* order, int32_t batch_size,
                           float lr, double* loss_sum, int64_t* n_correct, int where, float* kernel_ms);
/* the validation pass of spk.fit (d_vector.py:289): the forward kernel without the stash; nothing is updated (weights, gradients, m, v and t
 * keep their values) */
int ssp_lstm_trainer_evaluate(ssp_lstm_trainer* trainer, const float* X, const int32_t* labels, int64_t N, double* loss_sum, int64_t* n_correct,
                              int where, float* kernel_ms);
/* `tensor` (W: d_in x 4 units, U: units x 4 units, B: 4 units, WD: units x n_class, BD: n_class) of: the parameters, the LAST step's
 * gradients, Adam's m and v.  out: HOST.  Waits for the ctx stream.  A bias the network was created without answers SSP_ERR_INVALID. */
enum { SSP_LSTM_PARAM = 0, SSP_LSTM_GRAD = 1, SSP_LSTM_M = 2, SSP_LSTM_V = 3 };
enum { SSP_LSTM_W = 0, SSP_LSTM_U = 1, SSP_LSTM_B = 2, SSP_LSTM_WD = 3, SSP_LSTM_BD = 4 };
int ssp_lstm_trainer_read(ssp_lstm_trainer* trainer, int32_t what, int32_t tensor, float* out);
int ssp_lstm_trainer_steps(const ssp_lstm_trainer* trainer, int64_t* t); /* steps taken so far (Adam's t) */
/* measurement aid (tools/bench_lstm_train.py): ONE training step on the first batch_size rows of DEVICE arrays with a hipEvent between its
 * nine launches, then a host wait.  ms_out: HOST float[9] — forward with stash, Dense head, loss, dWd, dh_T, backward through time, dW + db,
 * dU, Adam.  The step counts: weights, m, v and t move as in ssp_lstm_trainer_epoch. */
int ssp_lstm_trainer_step_times(ssp_lstm_trainer* trainer, const float* X, const int32_t* labels, int32_t batch_size, float lr, float* ms_out);

/* ---- conv + GRU d-vector network training (since without a version step, like the entries above): nn_model.inference_gru,
 *      d_vector.py:213-269 — the network the reference's __main__ evaluates (:389).  ReduceLROnPlateau, CSVLogger and spkModel.save stay with
 *      the host side (d_vector.nn_model.inference_gru).  Unpinned: the reference tree holds no weights, logs or outputs of this network and
 *      Keras is not a dependency; the arithmetic is restated from Keras 2's sources and corroborated against torch.autograd only.  All
 *      fp32, the products on the exact-fp32 MFMA, no floating-point atomic anywhere.
 *        Network  Conv2D(F, (kh, kw), strides, `same`, linear, one input channel) on the (T, D) chunk (ssp_conv2d_same_forward's
 *                 arithmetic; To = ceil(T / sh) steps of Do F features, Do = ceil(D / sw)) -> TimeDistributed(Flatten) -> n_gru x
 *                 GRU(units, return_sequences) -> mean over time (t ascending) -> Dense(E), linear -> K.l2_normalize (eps 1e-12) ->
 *                 Dense(n_class) softmax.  Reference values: F 64, 5 x 5, strides 2, T 98, D 13 (49 steps of 448 features), 3 x 1024,
 *                 E 512, batch 128, Adam lr 1e-4.
 *        Regulariser  the convolution kernel carries regularizers.l2() with Keras' default factor lambda = 0.01: a step's loss is the
 *                 batch's mean cross-entropy + lambda sum K^2, dK gains 2 lambda K, and both the training and the validation loss sums
 *                 contain the term as Keras reports them: a batch of B rows adds B lambda sum K^2, K as it was before that step's
 *                 update.  Biases are not regularised.
 *        GRU cell the forward pass's, as stated for ssp_gru_forward above, with reset_after = 0 (what the reference's stand-alone Keras
 *                 runs); recurrent_activation 0 hard_sigmoid | 1 sigmoid.  reset_after = 1 is NOT trained: create answers
 *                 SSP_ERR_UNSUPPORTED for it before any GPU work.
 *        Backward through time, for t = To-1 .. 0; dh_t = the gradient from above (dmean / To for the top layer, the upper layer's dx_t
 *                 otherwise) + the recurrent part carried from step t + 1:
 *                   dhh = dh_t (1 - z);   da_h = dhh (1 - hh^2);   da_z = dh_t (h_{t-1} - hh) s'(z)
 *                   G   = da_h U_h^T;     da_r = (G . h_{t-1}) s'(r)
 *                   dh_{t-1} = dh_t z + G . r + [da_z | da_r] [U_z | U_r]^T
 *                   dW += x_t^T [da_z | da_r | da_h];   db += column sums of the same
 *                   dU_z,r += h_{t-1}^T [da_z | da_r];  dU_h += (r . h_{t-1})^T da_h
 *                   dx_t = [da_z | da_r | da_h] W^T
 *                 sigmoid: s'(s) = s (1 - s).  hard_sigmoid: s' = 0.2 where the fp32 activation lies strictly inside (0, 1) and 0
 *                 elsewhere (the LSTM trainer's rule).
 *        Around the GRUs  mean over time and Dense backward; l2_normalize backward with n = sqrt(max(sum x^2, eps)): dx = (dy - y (y . dy))
 *                 / n where sum x^2 >= eps, dx = dy / n below it; conv backward: dK and db only (the input needs no gradient), the sum
 *                 over the B To Do output positions in 64 fixed chunks added in order.
 *        Loss, accuracy, Adam: the dense trainer's, in the words of its section — the gradient at the logits is (softmax - onehot) / B
 *                 with B the actual batch (the tail batch included), Keras 2's Adam with eps 1e-7 outside the root and t counted over
 *                 the whole fit, one Adam launch over flat parameter, gradient, m and v buffers.
 *        Determinism: the same seed, data and order give the same bits.  A sequence is one MFMA column in the recurrent kernels; every
 *                 sum over rows has a fixed partition and order.
 *      Time steps are ordered by the stream: two launches per step, layer and direction (16 units x 16 sequences per wave, 64 units per
 *      workgroup).  The stash (h, z, r, hh, r . h_{t-1} per layer), the projection, the gate gradients and the gradient at a layer's
 *      input are time-major in a workspace allocated at create: To max_batch (d0 + 6 Hmax + max(Hmax, d0) + 5 sum units) floats, 0.58 GB
 *      at the reference shape.  Above 4 GiB create answers SSP_ERR_UNSUPPORTED. ---- */
/* conv_K: HOST float[kh x kw x F] (Keras' (kh, kw, 1, F)), conv_b: HOST float[F] or NULL; kh, kw <= 7, F <= 256, strides 1 or 2.
 * units: HOST int32[n_gru], n_gru in [1, 4]; W[l]: HOST float[d_in x 3 units[l]] with d_in = Do F for l = 0 and units[l - 1] above;
 * U[l]: HOST float[units[l] x 3 units[l]]; bias: NULL, or bias[l]: HOST float[3 units[l]] or NULL; units a multiple of 16 up to 1024,
 * d_in up to 4096.  dense_W: HOST float[units[n_gru - 1] x E], dense_b: HOST float[E] or NULL, E <= 4096; head_W: HOST float[E x n_class],
 * head_b: HOST float[n_class] or NULL, n_class in [2, 4096].  T in [1, 1024], D in [1, 4096], max_batch in [1, 1024], To max_batch up to 2^19 rows.  A limit exceeded,
 * reset_after = 1 or a workspace above the cap answers SSP_ERR_UNSUPPORTED; a null kernel, a bad switch or a shape below 1 answers
 * SSP_ERR_INVALID; both before any GPU work. */
typedef struct ssp_gru_trainer ssp_gru_trainer;
int ssp_gru_trainer_create(ssp_ctx* ctx, int32_t T, int32_t D, int32_t kh, int32_t kw, int32_t F, int32_t sh, int32_t sw, const float* conv_K,
                           const float* conv_b, int32_t n_gru, const int32_t* units, const float* const* W, const float* const* U,
                           const float* const* bias, int32_t E, const float* dense_W, const float* dense_b, int32_t n_class, const float* head_W,
                           const float* head_b, int32_t recurrent_activation, int32_t reset_after, int32_t max_batch, ssp_gru_trainer** out);
int ssp_gru_trainer_destroy(ssp_gru_trainer* trainer);
/* One pass of spk.fit over the data (d_vector.py:264-265).  X: float[N x T x D], labels: int32[N], on the side `where` names; order,
 * batch_size, lr, the queued steps without a host wait, the per-step loss / correct slots read back ONCE, the refusals and t: as for
 * ssp_lstm_trainer_epoch.  loss_sum contains the regulariser's term. */
int ssp_gru_trainer_epoch(ssp_gru_trainer* trainer, const float* X, const int32_t* labels, int64_t N, const int64_t* order, int32_t batch_size,
                          float lr, double* loss_sum, int64_t* n_correct, int where, float* kernel_ms);
/* the validation pass, in chunks of max_batch rows: nothing is updated (weights, gradients, m, v and t keep their values) */
int ssp_gru_trainer_evaluate(ssp_gru_trainer* trainer, const float* X, const int32_t* labels, int64_t N, double* loss_sum, int64_t* n_correct,
                             int where, float* kernel_ms);
/* `tensor` of: the parameters, the LAST step's gradients, Adam's m and v, in Keras' layout.  out: HOST.  Waits for the ctx stream.  A bias
 * the network was created without, or a layer it does not have, answers SSP_ERR_INVALID. */
enum { SSP_GRUT_PARAM = 0, SSP_GRUT_GRAD = 1, SSP_GRUT_M = 2, SSP_GRUT_V = 3 };
enum { SSP_GRUT_CONV_K = 0, SSP_GRUT_CONV_B = 1, SSP_GRUT_GRU0_W = 2, SSP_GRUT_GRU0_U = 3, SSP_GRUT_GRU0_B = 4, /* layer i: 2 + 3 i .. */
       SSP_GRUT_DENSE_W = 14, SSP_GRUT_DENSE_B = 15, SSP_GRUT_HEAD_W = 16, SSP_GRUT_HEAD_B = 17 };
int ssp_gru_trainer_read(ssp_gru_trainer* trainer, int32_t what, int32_t tensor, float* out);
int ssp_gru_trainer_steps(const ssp_gru_trainer* trainer, int64_t* t); /* steps taken so far (Adam's t) */
/* measurement aid (tools/bench_gru_train.py): ONE training step on the first batch_size rows of DEVICE arrays with a hipEvent between its
 * launch kinds, then a host wait.  ms_out: HOST float[30] — [0] conv forward, [1] mean + Dense + l2_normalize + head, [2] loss +
 * regulariser, [3] their backward, [4] conv backward, [5] Adam + re-pack of U; then for GRU layer i at [6 + 6 i ..]: input projection, the
 * 2 To forward step launches, the 2 To backward step launches, dW + db, dU, dx (zero for absent layers).  The step counts. */
enum { SSP_GRUT_TIMES = 30 };
int ssp_gru_trainer_step_times(ssp_gru_trainer* trainer, const float* X, const int32_t* labels, int32_t batch_size, float lr, float* ms_out);

/* ---- d-vector cosine scoring: replaces the scipy cosine double loop + argmin
 *      (d_vector.py:315-319, 346-361) ---- */
/* X: float[N x d]; C: float[S x d]; dist_out (nullable): float[N x S] = clip(1 - cos, 0, 2);
 * argmin_out (nullable): int32[N] (first index on ties); min_out (nullable): float[N]. */
/* per-speaker centroids avg[s] = mean(X[labels == s]) with a float64 accumulator in row order (d_vector.py:310-313,
 * and nn_model.enroll d_vector.py:331 with one label).  X: float[N x d]; labels: int32[N] in [0, S); out: float[S x d]
 * (a speaker without rows gives NaN like numpy's mean of an empty slice). */
int ssp_centroids(ssp_ctx* ctx, const float* X, const int32_t* labels, int64_t N, int32_t d, int32_t S, float* out,
                  int where, float* kernel_ms);

int ssp_cosine_identify(ssp_ctx* ctx, const float* X, int64_t N, int32_t d, const float* C, int32_t S,
                        float* dist_out, int32_t* argmin_out, float* min_out, int where, float* kernel_ms);
/* the same with a choice of arithmetic.  precision 0: fp32-input MFMA (the parity path; ssp_cosine_identify).  precision 1: the sweep on
 * bf16 MFMA with every operand split hi + lo (three products per k-step, fp32 accumulation) keeping each embedding's two largest
 * cosines; rows whose two best are closer than twice a PROVEN bound on |cos(bf16x3) - cos(fp32 path)| for unit vectors
 * (3.01 * 2^-16 + 4 d 2^-23 1.02 + (d + 8) 2^-24 = 5.5e-5 at d = 16, 1.9e-4 at d = 256: bf16 rounds to nearest with unit roundoff u = 2^-8, a
 * two-term split leaves u^2 = 2^-16 of each operand behind and three such terms reach the product; then worst-case fp32 accumulation on
 * both paths; the last term for the two paths' different normalisation roundings: the derivation stands at cosine.hip cos_band),
 * and every row that meets a NaN or a zero norm, are scored again by the fp32 kernel from a device-side list (no host round trip in
 * between; with device pointers the call is asynchronous on the ctx stream — its scratch lives on the ctx — and the diagnostics
 * below fetch their counts when asked).  argmin_out is therefore the fp32 path's on EVERY row; min_out is within the bound
 * of it (exact on the re-scored rows).  precision 2: a cascade — a sweep on the hi parts alone (one product per k-step, bound
 * 2.01 * 2^-8 + 2 d 2^-23 1.01 + (d + 8) 2^-24 = 7.9e-3: each operand is off by u = 2^-8, cosine.hip cos_band1) first, its close calls to the
 * bf16x3 sweep, that one's to fp32: the same arg-min guarantee, three times fewer matrix instructions on well-separated data (how many rows
 * each later stage takes depends on the data); min_out is then only within 7.9e-3 of the fp32 path's on rows the first sweep decided.
 * Arg-min / minimum only: dist_out must be NULL; d <= 256.
 * Norms: every path normalises in float32 before anything else, so the result does not depend on the scale of a row or a centroid as long
 * as its sum of squares is a normal float32: norms between 2^-40 and 2^40 are tested against float64 (tests/test_cosine_instances_gpu.py)
 * and the result is specified for norms between 2^-60 and 2^60.  Beyond that the sum of squares loses precision, underflows to 0 or
 * overflows, and the row (or the centroid's column) is unspecified: it may come back as the NaN of a zero-norm or infinite row. */
int ssp_cosine_identify2(ssp_ctx* ctx, const float* X, int64_t N, int32_t d, const float* C, int32_t S, float* dist_out,
                         int32_t* argmin_out, float* min_out, int where, int precision, float* kernel_ms);
/* diagnostics: rows the last precision >= 1 call scored again in fp32; rows its precision-2 cascade handed to the bf16x3 sweep
 * (these wait for the ctx stream when the counts of a device-pointer call have not been read yet) */
int ssp_cosine_last_rescored(const ssp_ctx* ctx, int32_t* n_out);
int ssp_cosine_last_split_rows(const ssp_ctx* ctx, int32_t* n_out);
/* precision = 3 (auto; d_vector.py:315-319's arg-min with the fp32 path's result on every row, at the cost of the cheapest path): the
 * pilot is the first round of the cascade's bf16 sweep (one machine-filling set of waves, at most N / 8 rows): it lists its close calls
 * as the full sweep would and counts the rows closer than the bf16x3 band beside them; from those two shares the call goes on as the
 * cascade (2: the sweep continues behind the pilot's rows, nothing is computed twice), or starts over as the bf16x3 sweep (1) or — when
 * nearly every row is a close call — the fp32 sweep (0).  N < 8192, d > 256 and dist_out requests run as precision 0 without a pilot.
 * One host wait per call (the counts), also with device pointers.  ssp_cosine_last_auto: what the last such call chose and saw
 * (precision_used -1: no auto call yet). */
int ssp_cosine_last_auto(const ssp_ctx* ctx, int32_t* precision_used, int32_t* pilot_rows, int32_t* pilot_to_bf16x3, int32_t* pilot_to_fp32);

#ifdef __cplusplus
}
#endif
#endif /* SSP_H_ */
