/*
 * sprintz_mi355x.h -- C-ABI of libsprintz_mi355x.so: the Sprintz codec hot path
 * (forecast -> zigzag -> per-block nbits -> bit-pack -> RLE) on AMD MI355X
 * (gfx950), bit-exact with dblalock/sprintz cpp/Compress.
 *
 * Plain C: pointers and sizes only.  Two groups of entry points:
 *
 *  (1) Drop-in single-call API.  One symbol per reference function of
 *      cpp/Compress/sprintz.h:16-32, same argument meaning, same return
 *      values (ELEMENTS, -1 for ndims == 0, floor'ed for odd 16-bit byte
 *      lengths -- sprintz_xff_rle.cpp:554), HOST pointers in and out.
 *      The reference's functions have C++ linkage (default argument
 *      `write_size=true`): the library ALSO exports them under exactly those
 *      C++ signatures, i.e. the reference's own mangled names
 *      (sprintz_amd/csrc/dropin.cpp, declared in include/sprintz_dropin.hpp),
 *      so an object compiled against the reference's sprintz.h -- e.g. the
 *      lzbench fork, reference README.md:29 -- links against this library
 *      unchanged.  One call = one chunk = one wavefront's worth of work: it
 *      is correct, not fast.  See (2).
 *
 *  (2) Batched device API.  The unit of GPU parallelism is the CHUNK: an
 *      independent compress() call on a contiguous slice, exactly what
 *      lzbench's block-size option does (reference README.md:58 "1KB and
 *      10KB blocks").  Predictor state resets per chunk, so chunks are
 *      embarrassingly parallel.  DEVICE pointers, explicit hipStream_t
 *      (passed as void* so that this header needs no HIP include).
 *
 * All functions return 0 / a non-negative count on success and a negative
 * SPRINTZ_E_* code on failure.  There is NO CPU fallback anywhere in this
 * library: without a usable HIP device every entry point fails with
 * SPRINTZ_E_NO_DEVICE.
 */
#ifndef SPRINTZ_MI355X_H
#define SPRINTZ_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history (additive: a caller built against version n runs against any library with abi_version() >= n)
 *   1  round 1: the 8 drop-in entry points, the batched device API, the optional Huffman ("SPZH") and query stages
 *   2  round 2: set_option, *_layout, the Huff0 wire format (huf0_*), online_*, comm_* / gather_layout / layout_bases,
 *      the column-major and run-less codec entry points, the reference's mangled C++ names (sprintz_dropin.hpp)
 *   3  round 3: compress_batch_dense / compress_dense_tmp_bytes, SPRINTZ_OPT_DENSE_MODE, env SPRINTZ_MI355X_RCCL_SONAME
 *   4  round 3: compress_batch_colmajor_dense, SPRINTZ_OPT_SPLIT_LANES, SPRINTZ_OPT_ENC_PAIR
 *   5  round 4: SPRINTZ_OPT_HOST_WAIT, SPRINTZ_OPT_LAT_CHUNKS, SPRINTZ_OPT_HOST_STREAMS, SPRINTZ_OPT_REF_DECODER_QUIRK (the single-call entry points work on a mapped staging buffer: one wait per call)
 *   6  round 5: huf0_decompress_batch_hint, SPRINTZ_OPT_HUF0_SYNC_CHUNKS, SPRINTZ_MI355X_MAX_NDIMS 65535
 *   7  round 6: SPRINTZ_OPT_BLK_CHUNKS (block-parallel delta kernels); the batched entry points refuse shapes whose tail outgrows remaining_len;
 *      later, additively: huf0_exact_tmp_bytes / huf0_compress_batch_exact; query_windows, SPRINTZ_QUERY_WIN_MIN / _MAX / _SUM; gather_rows;
 *      dispatch_counts / dispatch_name, SPRINTZ_KF_*; filter_rows / filter_row_ids, SPRINTZ_FILTER_ALL / _ANY; select_rows; aggregate_rows, SPRINTZ_AGG_*;
 *      histogram_rows, SPRINTZ_HIST_MAX_COUNTERS; moments_rows, SPRINTZ_MOM_*; groupby_rows, SPRINTZ_GBY_*;
 *      extrema_rows, SPRINTZ_EXT_*; filter_linear / filter_linear_tmp_bytes; segment_rows / segment_count, SPRINTZ_SEG_*;
 *      float_rows, SPRINTZ_FLOAT_*; compress_batch_float / compress_batch_float_dense, SPRINTZ_QUANT_FLOOR;
 *      rolling_rows, SPRINTZ_ROLL_*; project_rows, SPRINTZ_PROJECT_*; cumulative_rows / cumulative_tmp_bytes, SPRINTZ_CUM_*;
 *      derive_rows / derive_rows_tmp_bytes, SPRINTZ_DERIVE_*; fir_rows / fir_rows_tmp_bytes */
#define SPRINTZ_MI355X_ABI_VERSION 7

/* codec ids */
#define SPRINTZ_CODEC_DELTA 0   /* sprintz_*_delta_*  (sprintz_delta_rle.cpp / sprintz_delta_lowdim.cpp) */
#define SPRINTZ_CODEC_XFF   1   /* sprintz_*_xff_*    (sprintz_xff_rle.cpp   / sprintz_xff_lowdim.cpp), FIRE */
/* the reference's older codecs without run-length coding: 6-byte header
 * {u32 len; u16 ndims}, general row-major layout for every ndims; accepted by every batched
 * entry point; decoded by the generic kernels */
#define SPRINTZ_CODEC_DELTA_NORLE   2   /* compress_rowmajor_delta_{8b,16b}  sprintz_delta.cpp:776-1391 */
#define SPRINTZ_CODEC_BITPACK_NORLE 3   /* compress_rowmajor_{8b,16b}: bit-packing only  sprintz_delta.cpp:64-773 */
#define SPRINTZ_CODEC_XFF_NORLE     4   /* compress8b_rowmajor_xff (8-bit only; 8-byte header)  sprintz_xff.cpp:35-626 */

/* error codes */
#define SPRINTZ_E_INVALID    (-1)   /* bad argument; also what the reference returns for ndims == 0 (sprintz.cpp:36) */
#define SPRINTZ_E_NO_DEVICE  (-2)   /* no HIP device / HIP runtime error at init */
#define SPRINTZ_E_HIP        (-3)   /* a HIP call failed (see sprintz_mi355x_last_error) */
#define SPRINTZ_E_UNSUPPORTED (-4)  /* ndims above SPRINTZ_MI355X_MAX_NDIMS (or above 512 where only the lane-group kernels exist) */
#define SPRINTZ_E_CORRUPT    (-5)   /* decoder: stream header disagrees with the arguments */

#define SPRINTZ_MI355X_MAX_NDIMS 65535  /* whatever the stream header's uint16 holds (format.h:36-45).  513 .. 65535: the four RLE codec pairs, row-major,
                                           no query (csrc/any_ndims.hip: one workgroup per chunk; from 2048 on in column tiles); everything else <= 512 */

/* Extra readable bytes the decoder may touch after the last stream byte and
 * the encoder after the last input element (aligned 8-byte windows; the
 * reference has the same kind of contract). */
#define SPRINTZ_MI355X_READ_SLACK 16

int         sprintz_mi355x_abi_version(void);
const char* sprintz_mi355x_last_error(void);     /* thread-local, never NULL; describes the last call of
                                                    this thread that returned a negative code */

/* Tuning knobs (process-wide, atomic).  Their initial values come from the environment, read once:
 *   SPRINTZ_OPT_NO_FAST           1 = route every call to the generic kernels (A/B runs, tests);
 *                                 env SPRINTZ_MI355X_NO_FAST
 *   SPRINTZ_OPT_CHUNKS_PER_GROUP  consecutive chunks one lane group of the headline decoder walks,
 *                                 1..64, default 1; env SPRINTZ_MI355X_CHUNKS_PER_GROUP
 *   SPRINTZ_OPT_DENSE_MODE        how sprintz_mi355x_compress_batch_dense builds the container: 1 (default) = inside the
 *                                 encode launch (csrc/compact_tail.h), 0 = encode, then scan + copy (A/B runs, tests);
 *                                 env SPRINTZ_MI355X_DENSE_MODE
 *   SPRINTZ_OPT_HUF0_BIG_BATCH    chunks from which the Huff0 reader's one-table stream kernel runs as 2-wave workgroups with
 *                                 64-byte stream pieces (the built defaults HUF0_BIG_WG = 2, HUF0_BIG_PLOG = 6) instead of single waves,
 *                                 which are faster while each has a SIMD to itself (16 chunks a wave, 1 024 SIMDs); default 16385,
 *                                 0 = always (tests)
 *   SPRINTZ_OPT_HUF0_SYNC_CHUNKS  batches of at most this many chunks run the Huff0 reader's stream stage as one wave per chunk with sixteen
 *                                 self-synchronising decoders per stream (csrc/huf0_sync.h: a stream's ~900-look-up chain becomes three passes
 *                                 over ~60: what counts while the chip has idle issue slots -- 86 -> 45 us at 1 250 chunks, even at 10 000); default 8192, 0 = never (A/B runs, tests);
 *                                 env SPRINTZ_MI355X_HUF0_SYNC_CHUNKS
 *   SPRINTZ_OPT_SPLIT_LANES       1 (default) = 8-bit row-major streams of 65 .. 80 columns decode on 32 lanes a chunk (a pair of
 *                                 adjacent columns + one single column per lane, two chunks a wavefront), 0 = on 64 lanes x 2
 *                                 columns like the other shapes up to 128 columns; 0 also sizes the LDS carve of 16-bit streams of
 *                                 65 .. 80 columns for 128 columns again instead of 80 (A/B runs, tests); env SPRINTZ_MI355X_SPLIT_LANES
 *   SPRINTZ_OPT_ENC_PAIR          chunks from which row-major streams of 5 .. 64 columns are encoded with two columns per lane (the
 *                                 65 .. 128-column kernel on 4 .. 32 lanes a chunk: fewer instructions per sample) instead of one (a
 *                                 chunk's latency is shorter: what counts for a handful of chunks); default 1024, 1 = always,
 *                                 0 = never (A/B runs, tests); env SPRINTZ_MI355X_ENC_PAIR
 *   SPRINTZ_OPT_HOST_STREAMS      streams the single-call entry points of ALL host threads share per device (each call waits for its own
 *                                 launches through an event); default 4, 0 = a private stream per thread; read when a thread makes its
 *                                 first call; env SPRINTZ_MI355X_HOST_STREAMS
 *   SPRINTZ_OPT_REF_DECODER_QUIRK 0 (default) = every decoder is the true inverse of the reference ENCODER; 1 = runs of 16-bit
 *                                 general-layout FIRE streams are replayed as the reference DECODER replays them (coefficient
 *                                 shifted by 4 instead of 12, odd columns reading the counters' high halves:
 *                                 sprintz_xff_rle.cpp:893-901) -- not lossless on streams whose runs start with a non-zero
 *                                 prediction, but sample-for-sample what sprintz_decompress_xff_16b of the reference returns;
 *                                 env SPRINTZ_MI355X_REF_DECODER_QUIRK
 *   SPRINTZ_OPT_LAT_CHUNKS        batches of at most this many chunks (both layouts, 1 .. 64 columns, chunks of at most 16 KB; single calls and batches of
 *                                 at most 64 chunks up to ~40 KB of uint16 / ~24 KB of uint8: what fits a workgroup's 150 KB of LDS) decode
 *                                 with one workgroup per chunk (csrc/decode_lat.h: a chunk's latency is what counts; a third as many from 17 columns on); default 2048,
 *                                 0 = never (A/B runs, tests); env SPRINTZ_MI355X_LAT_CHUNKS
 *   SPRINTZ_OPT_BLK_CHUNKS        batches of at least this many chunks of the DELTA codec take the block-parallel kernels (a thread per block and
 *                                 16-byte row piece / per 16 rows of a univariate stream; csrc/encode_blk.h, decode_blk.h) where the shape allows;
 *                                 0 = never, default 2049 (env SPRINTZ_MI355X_BLK_CHUNKS).  Same bytes either way.
 *   SPRINTZ_OPT_BLK_KERNELS       which of the round-6 delta kernels such batches take, a mask: 1 = the block-parallel general-layout encoder, 2 = the
 *                                 block-parallel general-layout decoder, 4 = the block-parallel univariate low-dim encoder, 8 = the piece-sequential
 *                                 general-layout decoder (csrc/decode_row.h; wins over 2) on the shapes it measured faster on (8-bit rows of at
 *                                 least 32 columns), 16 = ... on every shape it fits (tests); default 9: the ones that measured faster than the
 *                                 lane-per-column kernels on BASELINE's configurations (env SPRINTZ_MI355X_BLK_KERNELS)
 *   SPRINTZ_OPT_HOST_WAIT         how a single-call entry point waits for its launches: 0 (default) = spin (hipStreamSynchronize)
 *                                 while at most 4 callers (and at most half of the CPUs this process may use) are inside the library,
 *                                 otherwise sleep and poll a mapped host word that a one-thread kernel at the end of the call writes
 *                                 (no runtime wait: 64 threads on 16 CPUs get 4x the calls per second of either runtime wait; a
 *                                 thread that waits this way has its timer slack at 1 us, prctl(PR_SET_TIMERSLACK), for the duration of the wait -- its own value is put back before the call returns); 1 = always
 *                                 spin; 2 = always sleep and poll; env SPRINTZ_MI355X_HOST_WAIT */
#define SPRINTZ_OPT_NO_FAST 0
#define SPRINTZ_OPT_CHUNKS_PER_GROUP 1
#define SPRINTZ_OPT_DENSE_MODE 2
#define SPRINTZ_OPT_HUF0_BIG_BATCH 3
#define SPRINTZ_OPT_SPLIT_LANES 4
#define SPRINTZ_OPT_ENC_PAIR 5
#define SPRINTZ_OPT_HOST_WAIT 6
#define SPRINTZ_OPT_LAT_CHUNKS 7
#define SPRINTZ_OPT_HOST_STREAMS 8
#define SPRINTZ_OPT_REF_DECODER_QUIRK 9
#define SPRINTZ_OPT_HUF0_SYNC_CHUNKS 10
#define SPRINTZ_OPT_BLK_CHUNKS 11
#define SPRINTZ_OPT_BLK_KERNELS 12
int sprintz_mi355x_set_option(int option, int value);
/* The value an option has now -- what the environment gave it or the last successful sprintz_mi355x_set_option -- or SPRINTZ_E_INVALID for an
 * unknown option (no option's value is negative).  What holds only under the options it was built with, such as a zone map and
 * SPRINTZ_OPT_REF_DECODER_QUIRK, records them from here. */
int sprintz_mi355x_get_option(int option);

/* Which kernel family served a call (per process, atomic).  Every family writes the same bytes as every other, so the output of a call
 * cannot tell which one ran; these counters can.  A family is one of the alternatives a launch site chooses between: by shape,
 * alignment, batch size and the knobs above.  A family's counter goes up by one behind each launch of it that the runtime accepted;
 * a call that fails before its launch (SPRINTZ_E_INVALID, SPRINTZ_E_NO_DEVICE, ...) moves none.  Calls made during stream capture
 * count at capture time: replaying the graph launches the kernels again and counts nothing.  Host only -- one relaxed add per launch,
 * nothing inside a kernel -- and never reset: read them before and after, and look at the difference.
 *   decompress_batch and every call that decodes through it (the single calls, query_batch, query_windows, filter_rows, select_rows, aggregate_rows, histogram_rows, moments_rows, groupby_rows, extrema_rows, the column-major form):
 *     DEC_BIG (more than 2047 columns)  DEC_ANY (513 .. 2047)  DEC_VERBATIM (chunks shorter than a group: header check + copy)
 *     DEC_LAT (csrc/decode_lat.h)  DEC_ROW (decode_row.h)  DEC_BLK (decode_blk.h)  DEC_FAST (decode_fast.h)  DEC_UNI (decode_uni.h)
 *     DEC_GENERIC (decode_kernel.h)
 *   gather_rows: GATHER_FAST (decode_fast.h)  GATHER_GENERIC (decode_kernel.h)
 *   compress_batch, compress_batch_dense and every call that encodes through them:
 *     ENC_BIG  ENC_ANY  ENC_LAT (encode_lat.h)  ENC_BLK / ENC_BLK_UNI (encode_blk.h: general layout / univariate)
 *     ENC_PAIR / ENC_WIDE / ENC_SPLIT (encode_wide.h: 5 .. 64 columns, two a lane / 65 .. 128 columns / 8 bits, 65 .. 80 columns)
 *     ENC_FAST (encode_fast.h)  ENC_UNI (encode_uni.h)  ENC_GENERIC (encode_kernel.h)
 *   how a dense container was built: DENSE_FUSED (inside the encode launch, csrc/compact_tail.h; counted with the encoder's family)
 *     DENSE_VERBATIM (chunks shorter than a group: one copy kernel, no encoder)  DENSE_COMPACT (sprintz_mi355x_compact's scan + copy
 *     passes, whether compress_batch_dense or the caller started them)
 *   transform_decode*: TR_CHAIN (one pass, chained scan)  TR_WAVE (wave scans: two passes over the stream, one where it is a single
 *     run)  TR_LEVELS (the generic levels alone)
 *   online_unpack* of the dynamic-delta kinds: ON_CHAIN (one pass)  ON_THREE (tile, scan, decode: three launches)
 *   the Huff0 reader's stream stage: HUF0_BIG (SPRINTZ_OPT_HUF0_BIG_BATCH)  HUF0_SYNC (SPRINTZ_OPT_HUF0_SYNC_CHUNKS)  HUF0_DEFAULT
 * sprintz_mi355x_dispatch_counts writes the first min(capacity, SPRINTZ_KF_COUNT) counters to counts[] (which may be NULL where capacity
 * <= 0) and returns SPRINTZ_KF_COUNT; sprintz_mi355x_dispatch_name returns a family's short lower-case name ("dec_row"), NULL out of range.
 * New families are appended: the numbers below do not change. */
#define SPRINTZ_KF_DEC_BIG 0
#define SPRINTZ_KF_DEC_ANY 1
#define SPRINTZ_KF_DEC_VERBATIM 2
#define SPRINTZ_KF_DEC_LAT 3
#define SPRINTZ_KF_DEC_ROW 4
#define SPRINTZ_KF_DEC_BLK 5
#define SPRINTZ_KF_DEC_FAST 6
#define SPRINTZ_KF_DEC_UNI 7
#define SPRINTZ_KF_DEC_GENERIC 8
#define SPRINTZ_KF_GATHER_FAST 9
#define SPRINTZ_KF_GATHER_GENERIC 10
#define SPRINTZ_KF_ENC_BIG 11
#define SPRINTZ_KF_ENC_ANY 12
#define SPRINTZ_KF_ENC_LAT 13
#define SPRINTZ_KF_ENC_BLK 14
#define SPRINTZ_KF_ENC_BLK_UNI 15
#define SPRINTZ_KF_ENC_PAIR 16
#define SPRINTZ_KF_ENC_FAST 17
#define SPRINTZ_KF_ENC_WIDE 18
#define SPRINTZ_KF_ENC_SPLIT 19
#define SPRINTZ_KF_ENC_UNI 20
#define SPRINTZ_KF_ENC_GENERIC 21
#define SPRINTZ_KF_DENSE_FUSED 22
#define SPRINTZ_KF_DENSE_VERBATIM 23
#define SPRINTZ_KF_DENSE_COMPACT 24
#define SPRINTZ_KF_TR_CHAIN 25
#define SPRINTZ_KF_TR_WAVE 26
#define SPRINTZ_KF_TR_LEVELS 27
#define SPRINTZ_KF_ON_CHAIN 28
#define SPRINTZ_KF_ON_THREE 29
#define SPRINTZ_KF_HUF0_BIG 30
#define SPRINTZ_KF_HUF0_SYNC 31
#define SPRINTZ_KF_HUF0_DEFAULT 32
#define SPRINTZ_KF_COUNT 33
int         sprintz_mi355x_dispatch_counts(uint64_t* counts, int capacity);
const char* sprintz_mi355x_dispatch_name(int family);

/* ------------------------------------------------------------------------
 * (1) Drop-in single-call API (host pointers).  Replaces, one to one:
 *   sprintz_compress_delta_8b    sprintz.h:18 / sprintz.cpp:57
 *   sprintz_decompress_delta_8b  sprintz.h:20 / sprintz.cpp:75
 *   sprintz_compress_xff_8b      sprintz.h:22 / sprintz.cpp:98
 *   sprintz_decompress_xff_8b    sprintz.h:24 / sprintz.cpp:115
 *   sprintz_compress_delta_16b   sprintz.h:28 / sprintz.cpp:138
 *   sprintz_decompress_delta_16b sprintz.h:30 / sprintz.cpp:156
 *   sprintz_compress_xff_16b     sprintz.h:32 / sprintz.cpp:180
 *   sprintz_decompress_xff_16b   sprintz.h:34 / sprintz.cpp:197
 * `dest` capacity: the reference's callers allocate len*3/2+64 elements for
 * compression and len+64 for decompression (test/compress_testing.hpp:145-147);
 * this implementation writes at most sprintz_mi355x_compress_bound() bytes /
 * exactly the decoded elements (it never over-runs like the reference does).
 * write_size == 0 omits the 8-byte header (sprintz_xff_rle.cpp:119-127).
 * Re-entrant from any number of host threads on disjoint buffers, like the reference (sprintz.h: one call = one thread).
 * Cost of a call (MI355X, 10 KB of uint16 x 8): 25 us either way -- memcpy into the calling thread's mapped staging buffer,
 * ONE launch (the one-workgroup-per-chunk kernel reads and writes that buffer directly and ends by writing the call's ticket
 * into a mapped host word), the caller polls that word (no runtime wait), memcpy out; chunks whose working set does not fit a
 * workgroup's LDS (above ~40 KB of uint16 / ~24 KB of uint8 to decode, ~34 / ~24 KB to encode) or of more than 64
 * columns take a staging kernel + the batched kernels' lane-per-column form + a wait (a chunk's latency then grows with its
 * groups: ~1.2 us each).  A decoder writes what the STREAM says (header counts, run lengths): like the reference's, these
 * entry points take no destination size, so a damaged stream can announce more samples than the caller's buffer holds --
 * callers that do not trust their input use the batched API, whose chunk_len bounds every chunk's output.
 * The batched API below is the fast path.
 * ---------------------------------------------------------------------- */
int64_t sprintz_mi355x_compress_delta_8b (const uint8_t*  src, uint32_t len, int8_t*  dest, uint16_t ndims, int write_size);
int64_t sprintz_mi355x_compress_xff_8b   (const uint8_t*  src, uint32_t len, int8_t*  dest, uint16_t ndims, int write_size);
int64_t sprintz_mi355x_compress_delta_16b(const uint16_t* src, uint32_t len, int16_t* dest, uint16_t ndims, int write_size);
int64_t sprintz_mi355x_compress_xff_16b  (const uint16_t* src, uint32_t len, int16_t* dest, uint16_t ndims, int write_size);

int64_t sprintz_mi355x_decompress_delta_8b (const int8_t*  src, uint8_t*  dest);
int64_t sprintz_mi355x_decompress_xff_8b   (const int8_t*  src, uint8_t*  dest);
int64_t sprintz_mi355x_decompress_delta_16b(const int16_t* src, uint16_t* dest);
int64_t sprintz_mi355x_decompress_xff_16b  (const int16_t* src, uint16_t* dest);

/* Headerless decode (the reference's 5-argument kernel form,
 * sprintz_xff.h:56-58 / sprintz_xff_rle.cpp:1181-1190): needed for streams
 * written with write_size == 0. */
int64_t sprintz_mi355x_decompress_noheader(int codec, int elem_bytes, const void* src, void* dest,
                                           uint16_t ndims, uint32_t ngroups, uint16_t remaining_len);

/* The layer below sprintz.h: the same four codecs with the payload layout chosen by the caller
 * instead of by ndims.  Replaces compress_rowmajor_{delta,xff}_rle[_lowdim]_{8b,16b} and their
 * 2-argument decoders (sprintz_delta.h:49-91, sprintz_xff.h:43-85):
 *   SPRINTZ_LAYOUT_AUTO     what sprintz.h's dispatch picks (sprintz.cpp:34-50)
 *   SPRINTZ_LAYOUT_GENERAL  row-major payload for every ndims (the *_rle_* names)
 *   SPRINTZ_LAYOUT_LOWDIM   column-major low-dim payload; ndims <= 4 @8b / <= 2 @16b, else -1
 *                           (sprintz_delta_lowdim.cpp:64-70)
 * codec: SPRINTZ_CODEC_DELTA or SPRINTZ_CODEC_XFF. */
#define SPRINTZ_LAYOUT_AUTO 0
#define SPRINTZ_LAYOUT_GENERAL 1
#define SPRINTZ_LAYOUT_LOWDIM 2
int64_t sprintz_mi355x_compress_layout(int codec, int elem_bytes, const void* src, uint32_t len, void* dest, uint16_t ndims,
                                       int write_size, int layout);
int64_t sprintz_mi355x_decompress_layout(int codec, int elem_bytes, const void* src, void* dest, int layout);

/* ------------------------------------------------------------------------
 * (2) Batched device API (device pointers, asynchronous on `hip_stream`).
 * ---------------------------------------------------------------------- */

/* Worst-case compressed bytes of one chunk (a multiple of 128: slots of this stride start on 128-byte lines, and the
 * encoders flush whole lines). */
size_t sprintz_mi355x_compress_bound(int elem_bytes, uint32_t chunk_len, uint16_t ndims);

/* Number of chunks total_len splits into. */
uint64_t sprintz_mi355x_num_chunks(uint64_t total_len, uint32_t chunk_len);

/* Compress: d_src holds total_len elements, row-major [row][ndims]; chunk c
 * covers elements [c*chunk_len, min((c+1)*chunk_len, total_len)) and is
 * compressed exactly as sprintz_compress_<codec>_<w>b(src+c*chunk_len, n,
 * dest, ndims, true) would.  Chunk c's stream is written at
 * d_slots + c*slot_stride (slot_stride >= compress_bound, multiple of 16,
 * d_slots 16-byte aligned); d_sizes[c] receives its exact byte length and
 * d_rets[c] (optional, may be NULL) the reference's element-count return.
 * d_src must be readable for SPRINTZ_MI355X_READ_SLACK bytes past its end.
 * More than 2 047 columns: d_slots (and the decoder's d_out) must be ordinary DEVICE memory (hipMalloc) -- those
 * kernels build the stream with device-scope atomics on the slot and read their own output back; they also take
 * nchunks * ndims * 4 bytes of stream-ordered scratch (hipMallocAsync) per FIRE launch, so such a launch cannot be
 * captured into a graph.  From 4 096 columns on a shape whose verbatim tail can exceed the stream header's 16-bit
 * remaining_len (format.h:40; a chunk of whole blocks: 16 * ndims elements, else 8 * ndims + the ragged rest, or the
 * whole chunk when it is shorter than a group) is REFUSED with SPRINTZ_E_UNSUPPORTED by every batched entry point: the
 * reference's single call writes such a stream truncated (it decodes to a prefix), which the drop-in single-call
 * symbols reproduce and a batch must not. */
int sprintz_mi355x_compress_batch(int codec, int elem_bytes,
                                  const void* d_src, uint64_t total_len, uint32_t chunk_len, uint16_t ndims,
                                  void* d_slots, size_t slot_stride,
                                  uint32_t* d_sizes, int64_t* d_rets, void* hip_stream);

/* Compact slot-strided chunk streams into one dense buffer: exclusive scan of
 * sizes -> d_offsets[0..nchunks] (d_offsets[nchunks] = total bytes), then a
 * coalesced copy.  `align` (power of two, 1..16) rounds every chunk start up;
 * align=1 gives the byte-dense concatenation.  d_dense capacity must be
 * >= sum(round_up(size, align)) + SPRINTZ_MI355X_READ_SLACK.
 * d_scan_tmp: scratch of sprintz_mi355x_compact_tmp_bytes(nchunks) bytes. */
size_t sprintz_mi355x_compact_tmp_bytes(uint64_t nchunks);
int sprintz_mi355x_compact(const void* d_slots, size_t slot_stride, const uint32_t* d_sizes,
                           uint64_t nchunks, uint32_t align,
                           void* d_dense, uint64_t* d_offsets, void* d_scan_tmp, void* hip_stream);

/* Compress straight into the dense container: sprintz_mi355x_compress_batch followed by
 * sprintz_mi355x_compact(align = 16), with the same results in d_sizes / d_rets / d_dense / d_offsets -- but for the
 * shapes the fast encoder takes (general layout, ndims <= 64, 16-byte aligned blocks) in ONE launch: every workgroup
 * finds its place in the container by a chained scan over workgroups and copies its own chunks slot -> container before
 * it exits (csrc/compact_tail.h).  d_slots is still needed (the streams pass
 * through it); d_tmp: sprintz_mi355x_compress_dense_tmp_bytes(nchunks) bytes, 8-byte aligned; d_dense: 16-byte aligned,
 * capacity as for sprintz_mi355x_compact.  Other shapes run the two launches internally. */
size_t sprintz_mi355x_compress_dense_tmp_bytes(uint64_t nchunks);
int sprintz_mi355x_compress_batch_dense(int codec, int elem_bytes,
                                        const void* d_src, uint64_t total_len, uint32_t chunk_len, uint16_t ndims,
                                        void* d_slots, size_t slot_stride, uint32_t* d_sizes, int64_t* d_rets,
                                        void* d_dense, uint64_t* d_offsets, void* d_tmp, void* hip_stream);

/* Decompress: chunk c's stream occupies [d_offsets[c], d_offsets[c+1]) of d_comp
 * (any byte alignment; d_offsets has nchunks+1 entries, the last one being the
 * end of the last stream -- the layout sprintz_mi355x_compact produces; padding
 * between streams is allowed) and is decoded exactly as
 * sprintz_decompress_<codec>_<w>b would, to d_out + c*chunk_len elements.  d_rets[c] (optional) receives the
 * element count decoded (the reference's return value), or a negative
 * SPRINTZ_E_* if the stream header's ndims differs from `ndims`.
 * d_comp must be readable for SPRINTZ_MI355X_READ_SLACK bytes past the last
 * stream byte. */
int sprintz_mi355x_decompress_batch(int codec, int elem_bytes,
                                    const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                                    uint32_t chunk_len, uint16_t ndims,
                                    void* d_out, int64_t* d_rets, void* hip_stream);

/* ------------------------------------------------------------------------
 * (3) Optional Huffman stage over the container (bytes as symbols, after
 * bit-packing -- what the paper does with Huff0, communicate/ubicomp/
 * method.tex:293-297).  The reference tree contains NO Huffman coder
 * (SURVEY.md 8c), so this container format is this library's own (specified in
 * oracle/huf_oracle.c: 64-chunk segments share a code table, 4 byte-aligned
 * sub-streams per chunk, 11-bit code limit) and its parity is unpinned; the
 * Sprintz streams it wraps remain bit-exact with the reference.
 *   d_tables : ceil(nchunks/64) * 128 bytes of code-length tables
 *   d_huf    : capacity >= sprintz_mi355x_huf_bound(sum of d_sizes, nchunks)
 *   d_tmp    : sprintz_mi355x_huf_tmp_bytes(nchunks) bytes of scratch
 * ---------------------------------------------------------------------- */
size_t sprintz_mi355x_huf_tmp_bytes(uint64_t nchunks);
size_t sprintz_mi355x_huf_bound(uint64_t total_stream_bytes, uint64_t nchunks);
/* container (d_dense, d_offsets[nchunks+1], d_sizes[nchunks] = exact stream bytes)
 * -> Huffman records at d_huf + d_huf_offsets[c] (d_huf_offsets[nchunks] = total).
 * A segment's byte counts are added in 32 bits (the oracle's in 64): 64 consecutive chunks must total less than 4 GiB. */
int sprintz_mi355x_huf_compress_batch(const void* d_dense, const uint64_t* d_offsets, const uint32_t* d_sizes,
                                      uint64_t nchunks, void* d_huf, uint64_t* d_huf_offsets, void* d_tables,
                                      void* d_tmp, void* hip_stream);
/* inverse: rebuilds the container with chunk starts rounded up to `align`
 * (fills d_offsets[nchunks+1] and d_sizes[nchunks]); feed it to
 * sprintz_mi355x_decompress_batch.  d_dense holds dense_capacity bytes; a
 * record that is damaged (does not fit its slot of the container, or whose
 * output would not fit d_dense) decodes to nothing and gets
 * d_rets[c] = SPRINTZ_E_CORRUPT (d_rets optional; otherwise the chunk's byte
 * count) -- damaged input never makes the kernels read or write out of bounds. */
int sprintz_mi355x_huf_decompress_batch(const void* d_huf, const uint64_t* d_huf_offsets, const void* d_tables,
                                        uint64_t nchunks, uint32_t align, void* d_dense, uint64_t dense_capacity,
                                        uint64_t* d_offsets, uint32_t* d_sizes, int64_t* d_rets, void* d_tmp,
                                        void* hip_stream);

/* ------------------------------------------------------------------------
 * Column-major matrices (BASELINE.json config 5: "uint16 colmajor, 32
 * variables").  The matrix X[nrows][ndims] lives in HBM column by column:
 * element (r, d) at base[d * col_stride + r].  Chunk c holds rows
 * [c*rows_per_chunk, min((c+1)*rows_per_chunk, nrows)) and its stream is
 * byte-for-byte what the reference's compress() produces for the row-major
 * flattening of those rows (len = rows * ndims) -- the transposition happens
 * in the kernels' addressing (a lane owns a column, so its 8 samples of a
 * block are one contiguous 16-byte piece), not in memory.
 *   compress:   col_stride >= nrows
 *   decompress: col_stride >= nchunks * rows_per_chunk (ragged last chunk:
 *               rows past nrows are not written by a valid stream)
 * Containers are interchangeable with the row-major entry points.
 * Any col_stride is taken: the lane-per-column kernels serve strides of whole
 * blocks (a multiple of 8, with rows_per_chunk a multiple of 8 and a 16-byte
 * aligned base) within their 32-bit reach -- compress: col_stride < 2^32
 * elements; decompress: ndims * col_stride * elem_bytes < 0xf0000000 -- and
 * everything else falls back to the generic kernels, which address every
 * element at 64 bits.  Same streams, same matrix, either way.
 * ---------------------------------------------------------------------- */
int sprintz_mi355x_compress_batch_colmajor(int codec, int elem_bytes, const void* d_src, uint64_t nrows, uint64_t col_stride,
                                           uint32_t rows_per_chunk, uint16_t ndims, void* d_slots, size_t slot_stride,
                                           uint32_t* d_sizes, int64_t* d_rets, void* hip_stream);
/* the column-major write path in one call: streams + the 16-byte aligned container + offsets[nchunks + 1], as
 * sprintz_mi355x_compress_batch_dense does for row-major data (same d_tmp size, same fallback to encode + scan + copy for
 * the shapes whose encoder carries no container tail) */
int sprintz_mi355x_compress_batch_colmajor_dense(int codec, int elem_bytes, const void* d_src, uint64_t nrows, uint64_t col_stride,
                                                 uint32_t rows_per_chunk, uint16_t ndims, void* d_slots, size_t slot_stride,
                                                 uint32_t* d_sizes, int64_t* d_rets, void* d_dense, uint64_t* d_offsets, void* d_tmp,
                                                 void* hip_stream);
int sprintz_mi355x_decompress_batch_colmajor(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets,
                                             uint64_t nchunks, uint32_t rows_per_chunk, uint16_t ndims, uint64_t col_stride,
                                             void* d_out, int64_t* d_rets, void* hip_stream);

/* ------------------------------------------------------------------------
 * Query on compressed data.  Replaces
 *   query_rowmajor_delta_rle_{8b,16b}(src, dest, const QueryParams&)  cpp/Compress/sprintz_delta.h:95-98
 *   query_rowmajor_xff_rle_{8b,16b}(src, dest, const QueryParams&)    cpp/Compress/sprintz_xff.h:90-93
 *   QueryParams{op, materialize}, QueryTypes::{NOOP,REDUCE_MAX,REDUCE_SUM}  cpp/Compress/query.hpp:23-29
 * The reduction is fused into the decode kernel: with materialize == 0 nothing
 * but the per-column results leaves the chip.
 *
 * Semantics.  The reference computes its reductions into a local object and
 * throws them away (sprintz_xff_rle_query.cpp:69-104: DUMMY_READ_QUERY_RESULT),
 * and its functors are unfinished (query.hpp:222 writes every stripe's maximum
 * to state[0]; query.hpp:84-87,120-123 shift the wrong way and drop columns
 * 8..15 of every 32), so there is no reference RESULT to be bit-exact with.
 * Defined here: for column c (element index mod ndims), over ALL decompressed
 * elements of the chunk including its verbatim tail --
 *   op 1 (REDUCE_MAX): the unsigned maximum;  op 2 (REDUCE_SUM): the sum of the
 *   unsigned values, in 64 bits.
 * The materialised output is bit-exact with decompress (which is what the
 * reference's own query tests assert, test/test_query.cpp:59-120,180-200).
 *
 *   op          : SPRINTZ_QUERY_NOOP / _MAX / _SUM
 *   materialize : 0 = do not write the decompressed data (d_out may be NULL)
 *   flags       : SPRINTZ_QUERY_GENERAL_LAYOUT = the stream uses the general
 *                 row-major layout whatever ndims is, as the reference's
 *                 *_rowmajor_*_rle_* functions do (sprintz.h's dispatch uses the
 *                 low-dim layout for ndims <= 4 @8b / <= 2 @16b; that is the default)
 *   d_partials  : [nchunks][ndims] uint64, per-chunk per-column results
 *   d_rets      : optional, as in decompress_batch
 * sprintz_mi355x_query_reduce folds the partials over the chunks:
 *   d_result[ndims] = max / sum over chunks.
 * ---------------------------------------------------------------------- */
#define SPRINTZ_QUERY_NOOP 0
#define SPRINTZ_QUERY_MAX 1
#define SPRINTZ_QUERY_SUM 2
#define SPRINTZ_QUERY_GENERAL_LAYOUT 1u
int sprintz_mi355x_query_batch(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                               uint32_t chunk_len, uint16_t ndims, int op, int materialize, uint32_t flags, void* d_out,
                               uint64_t* d_partials, int64_t* d_rets, void* hip_stream);
int sprintz_mi355x_query_reduce(int op, const uint64_t* d_partials, uint64_t nchunks, uint16_t ndims, uint64_t* d_result,
                                void* hip_stream);

/* Windowed query: per-window min / max / sum of every column, fused into the decode, nothing else leaving the chip.
 * The paper stores series in small segments so that queries over arbitrary time intervals are cheap
 * (communicate/intro.tex:55) and plans "sliding mean on 8b data" and "max on 16b data" (communicate/results.tex:265-272);
 * the ops are those of QueryParams (cpp/Compress/query.hpp:23-29) plus the minimum, per window instead of per chunk.
 *
 * The batch is given exactly as to sprintz_mi355x_query_batch (codec, elem_bytes, container, offsets, nchunks, chunk_len,
 * ndims, flags: SPRINTZ_QUERY_GENERAL_LAYOUT).  With D = ndims, R = ceil(chunk_len / D) rows a chunk slot,
 * W = window_rows (a multiple of 8, at least 8) and nwin = ceil(R / W): element e of chunk c (0 <= e < the element count its
 * stream header gives) is in column e % D and window (e / D) / W -- windows are relative to the chunk.  For chunk c,
 * window w and column d the call writes, at index (c*nwin + w)*D + d,
 *   d_min: the unsigned minimum, element type (uint8 / uint16)      (ops & SPRINTZ_QUERY_WIN_MIN)
 *   d_max: the unsigned maximum, element type                      (ops & SPRINTZ_QUERY_WIN_MAX)
 *   d_sum: the sum, uint64                                         (ops & SPRINTZ_QUERY_WIN_SUM)
 * over the samples sprintz_mi355x_decompress_batch would write under the same options (SPRINTZ_OPT_REF_DECODER_QUIRK
 * included; the verbatim tail and a partial last row count).  A window without elements -- in a short last chunk, or in
 * any chunk whose stream holds fewer rows than its slot -- holds the identities: min 0xFF / 0xFFFF, max 0, sum 0.  Every
 * one of the nchunks*nwin*D entries of each selected output is written; an output not selected may be NULL.
 * d_rets (optional) as in decompress_batch: elements decoded, or < 0 for a damaged chunk, whose entries are then
 * unspecified -- nothing is written outside them, and every other chunk's are exact.
 * Returns SPRINTZ_E_INVALID for a window_rows that is not a multiple of 8 >= 8, ops outside 1..7, a selected output that
 * is NULL, a selected d_min / d_max not aligned to the element size or d_sum not to 8 bytes, an unknown flag; SPRINTZ_E_UNSUPPORTED
 * for more than 512 columns -- all before the device is touched. */
#define SPRINTZ_QUERY_WIN_MIN 1u
#define SPRINTZ_QUERY_WIN_MAX 2u
#define SPRINTZ_QUERY_WIN_SUM 4u
int sprintz_mi355x_query_windows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                                 uint32_t chunk_len, uint16_t ndims, uint32_t window_rows, uint32_t ops, uint32_t flags,
                                 void* d_min, void* d_max, uint64_t* d_sum, int64_t* d_rets, void* hip_stream);
/* Filter rows: which rows satisfy a condition on their columns?  One bit per row and one count per chunk, fused into the decode:
 * nothing but the mask and the counts leaves the chip.  With sprintz_mi355x_filter_row_ids and sprintz_mi355x_gather_rows it is
 * "find the rows, then fetch them" without ever materialising the batch.
 *
 * The batch is given exactly as to sprintz_mi355x_query_batch (codec, elem_bytes, container, offsets, nchunks, chunk_len,
 * ndims, flags: SPRINTZ_QUERY_GENERAL_LAYOUT and nothing else).  With D = ndims, R = ceil(chunk_len / D) rows a chunk slot and
 * MB = ceil(R / 8) mask bytes a chunk slot: element e of chunk c is in row e / D and column e % D, and row r of chunk c EXISTS if
 * all D of its elements lie inside the element count the chunk's stream header gives -- a partial last row is not a row.
 * d_lo, d_hi: device arrays of ndims elements of the element type.  Comparison is unsigned and inclusive; lo[d] > hi[d] means
 * "column d never matches" (the neutral element of ANY), 0 .. 0xFF / 0 .. 0xFFFF "always matches" (the neutral element of ALL).
 * A row matches, under SPRINTZ_FILTER_ALL, if every column d has lo[d] <= x <= hi[d]; under SPRINTZ_FILTER_ANY, if some column has.
 *   d_mask  : bit r & 7 of d_mask[c*MB + (r >> 3)] is 1 iff row r of chunk c exists and matches, judged on the values
 *             sprintz_mi355x_decompress_batch would write under the same options (SPRINTZ_OPT_REF_DECODER_QUIRK included; the
 *             verbatim tail counts, and so does a chunk without groups).  Every one of the nchunks*MB bytes is written; bits of rows
 *             that do not exist are 0 -- a row that does not exist never matches, whatever the bounds.  When chunk_len % D == 0 and
 *             R % 8 == 0 the mask is the batch's rows in order, little-endian bit order.
 *   d_counts: d_counts[c] = the number of set bits of chunk c.
 * d_mask or d_counts may be NULL, not both.  d_rets (optional) as in decompress_batch: elements decoded, or < 0 for a damaged
 * chunk, whose mask bytes and count are then unspecified -- nothing is written outside them, and every other chunk is exact.
 * The call does not read the bounds on the host, does not synchronise and does not allocate.  Its launch counts under DEC_FAST,
 * DEC_UNI or DEC_GENERIC, as query_windows' does.
 * Returns, before the device is touched: SPRINTZ_E_INVALID for an unknown mode or flag, a NULL d_lo / d_hi / d_comp / d_offsets,
 * both outputs NULL, d_lo / d_hi not aligned to the element size, d_counts not aligned to 4 bytes, d_rets not aligned to 8 bytes,
 * chunk_len outside 1..2^30; SPRINTZ_E_UNSUPPORTED for more than 512 columns and for the non-RLE codecs.  nchunks == 0 returns 0
 * and launches nothing. */
#define SPRINTZ_FILTER_ALL 0u   /* a row matches if EVERY column d has lo[d] <= x <= hi[d] */
#define SPRINTZ_FILTER_ANY 1u   /* ... if SOME column has */
int sprintz_mi355x_filter_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                               uint32_t chunk_len, uint16_t ndims, const void* d_lo, const void* d_hi, uint32_t mode,
                               uint32_t flags, uint8_t* d_mask, uint32_t* d_counts, int64_t* d_rets, void* hip_stream);
/* Linear filter rows: the second producer of a row mask.  filter_rows' predicate is a box, column by column; this one relates
 * columns ("a > b", "x + y + z > t") and a row to the row in front of it ("|x[r] - x[r-1]| > t", "state[r] != state[r-1]") -- one
 * linear form over a row and its predecessor, tested against an interval.  The batch is given as to filter_rows, with
 * chunk_len % ndims == 0: chunk c holds batch rows [c R, (c + 1) R), R = chunk_len / ndims; a partial last row of the batch is not a
 * row.  For batch row g, with x the unsigned element widened to 32 bits:
 *
 *     s(g) = bias + sum_d w[d] x[g, d] + sum_d u[d] x[p(g), d],   p(g) = g - 1 for g > 0, p(0) = 0
 *     row g matches  <=>  lo <= s(g) <= hi
 *
 * Row 0 is its own predecessor (numpy.diff(..., prepend=x[0])).  w = d_weights and u = d_lag_weights are device arrays of ndims
 * int32; d_lag_weights == NULL means no lag term.  bias, lo and hi are int32; the comparison is signed and inclusive, and lo > hi
 * matches nothing.  THE WRAPPING RULE: s is computed in wrapping 32-bit two's-complement arithmetic.  The library cannot see weights
 * that live on the device, so it cannot refuse a form that wraps: s is the exact integer wherever
 *     B = |bias| + (2^W - 1) sum_d (|w[d]| + |u[d]|) < 2^31        (W = 8 elem_bytes),
 * and a caller who wants exact answers keeps B below 2^31 (the Python layer refuses the others).
 * d_mask, d_counts, d_rets: filter_rows' outputs, in its layout -- MB = ceil(R / 8) bytes a chunk, 0 for rows that do not exist;
 * d_mask or d_counts may be NULL, not both.  The masks of both filters combine bytewise (AND, OR) and feed select_rows and the
 * other mask consumers unchanged.
 * d_tmp: with d_lag_weights, sprintz_mi355x_filter_linear_tmp_bytes(elem_bytes, nchunks, ndims) bytes of device scratch, aligned to 8
 * (the layout is the library's own; the contents need not be kept); else ignored.  Inside the decode launch a chunk's first row is
 * its own predecessor; a second small launch on the same stream then gives row 0 of every chunk behind the first its true
 * predecessor, the last row of the chunk in front.  Row 0 of a chunk that follows a damaged chunk is unspecified; d_rets names the
 * damaged one.  The launch counts under DEC_FAST or DEC_GENERIC.
 * Returns, before the device is touched: SPRINTZ_E_INVALID for an unknown flag, a NULL d_comp / d_offsets / d_weights, both outputs
 * NULL, chunk_len % ndims != 0 (or outside 1..2^30), d_weights / d_lag_weights / d_counts not aligned to 4 bytes, d_rets not aligned
 * to 8, d_tmp NULL or not aligned to 8 while d_lag_weights is given; SPRINTZ_E_UNSUPPORTED for more than 512 columns and for the
 * non-RLE codecs.  nchunks == 0 returns 0 and launches nothing.  _tmp_bytes returns 0 for bad arguments. */
int sprintz_mi355x_filter_linear(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                                 uint32_t chunk_len, uint16_t ndims, const int32_t* d_weights, const int32_t* d_lag_weights,
                                 int32_t bias, int32_t lo, int32_t hi, uint32_t flags, void* d_tmp, uint8_t* d_mask, uint32_t* d_counts,
                                 int64_t* d_rets, void* hip_stream);
uint64_t sprintz_mi355x_filter_linear_tmp_bytes(int elem_bytes, uint64_t nchunks, uint16_t ndims);
/* A mask of filter_rows as batch row numbers.  Needs chunk_len % ndims == 0, as gather_rows does: with R = chunk_len / D, batch row g
 * is row g % R of chunk g / R, and d_mask holds MB = ceil(R / 8) bytes a chunk.  d_bases[c] is the exclusive prefix sum of the
 * chunks' counts, computed by the caller (torch.cumsum, hipcub, ...).  The i-th set bit of chunk c, in ascending row order, writes
 * c*R + r to d_ids[d_bases[c] + i]; a position >= capacity is dropped.  Each entry has exactly one writer: no atomics, and the
 * output is deterministic -- ascending where the bases are the prefix sums.  Bits of rows >= R in a chunk's last byte are ignored.
 * Returns, before the device is touched: SPRINTZ_E_INVALID for chunk_len % ndims != 0 (or ndims == 0, chunk_len outside 1..2^30),
 * NULL pointers with nchunks > 0, d_bases / d_ids not aligned to 8 bytes.  nchunks == 0 returns 0 and launches nothing. */
int sprintz_mi355x_filter_row_ids(const uint8_t* d_mask, const uint64_t* d_bases, uint64_t nchunks, uint32_t chunk_len,
                                  uint16_t ndims, uint64_t* d_ids, uint64_t capacity, void* hip_stream);
/* Zone maps: skip the chunks a filter's bounds already decide.  A filter decodes every chunk, however selective it is; a chunk's
 * per-column minimum and maximum prove, for most range predicates on slowly drifting series, that none of its rows can match or that
 * all of them do.  Build the map once (zone_map), then for every query: prune (classify the chunks and compact the offsets of those that
 * still need the decoder), run sprintz_mi355x_filter_rows / _filter_linear on (d_comp, d_surv_offsets, n') into compact outputs, and
 * expand them into the filter's own layout.  The result is bit for bit the unpruned call's.  The compacted offsets are a valid container
 * for every decoder: a chunk's stream is read as offsets[c+1] - offsets[c] bytes, the header allows padding behind a stream, and the
 * skipped chunks are that padding.
 *
 * zone_map: for chunk c and column d, d_zmin / d_zmax [nchunks][ndims] (element type) take the unsigned minimum and maximum over every
 * element sprintz_mi355x_decompress_batch would write for the chunk (the verbatim tail and a partial last row count; a chunk without
 * elements holds the identities, min 0xFF / 0xFFFF and max 0), and d_zlen[c] (int64) the chunk's element count, or < 0 for a damaged
 * chunk, whose entries are unspecified.  It is exactly sprintz_mi355x_query_windows with one window a chunk (window_rows = the rows of
 * a chunk slot rounded up to 8), ops MIN | MAX and d_rets = d_zlen -- a contract of its own so that a later encoder can fill it while
 * it compresses.  A zone map describes the container as it was when the map was built, under the flags (SPRINTZ_QUERY_GENERAL_LAYOUT)
 * and the SPRINTZ_OPT_REF_DECODER_QUIRK state it was built with: pruning a changed container, or under another layout or quirk state,
 * is the caller's error and goes unnoticed.  Returns as query_windows does, and SPRINTZ_E_INVALID for a NULL output or a d_zlen not
 * aligned to 8 bytes -- all before the device is touched.
 *
 * zone_prune_box (filter_rows' predicate: d_lo, d_hi, mode) and zone_prune_linear (filter_linear's without a lag term: d_weights, bias,
 * lo, hi; chunk_len % ndims == 0) share one output set:
 *   d_class[nchunks] uint8   : 0 NONE -- no row of the chunk matches; 1 ALL -- every existing row matches; 2 DECODE -- the decoder must look.
 *   d_pos[nchunks + 1] uint64: the number of DECODE chunks in front of chunk c; d_pos[nchunks] = n', the survivors.
 *   d_surv_offsets[nchunks + 1] uint64: entry d_pos[c] = d_offsets[c] for every DECODE chunk, ascending; entries n' .. nchunks =
 *                              d_offsets[nchunks], so (d_comp, d_surv_offsets, n') is a container of the survivors.
 * With rows_c = zlen[c] / ndims: zlen[c] < 0 is DECODE (its place among the survivors keeps every other chunk's place; expand reports it with the map's code); else rows_c == 0 is NONE; else
 *   box, unsigned and inclusive: column d is DISJOINT if lo[d] > hi[d], zmax < lo[d] or zmin > hi[d], and INSIDE if lo[d] <= zmin and
 *     zmax <= hi[d].  SPRINTZ_FILTER_ALL: NONE if some column is disjoint, else ALL if every column is inside.  SPRINTZ_FILTER_ANY: ALL if
 *     some column is inside, else NONE if every column is disjoint.  Otherwise DECODE.
 *   linear: in 64-bit arithmetic smin = bias + sum_d (w[d] >= 0 ? w[d] zmin[d] : w[d] zmax[d]) and smax its mirror.  A range that leaves
 *     int32 is DECODE (filter_linear's 32-bit sum may wrap there, and only the decoder knows what it yields); else NONE if lo > hi,
 *     smax < lo or smin > hi; ALL if lo <= smin and smax <= hi; otherwise DECODE.
 * THE 4 GiB RULE: the decoders address the streams of one wavefront as 32-bit offsets from the wavefront's first stream, and compaction
 * can put distant chunks into one wavefront: if d_offsets[nchunks] - d_offsets[0] >= 0xf0000000, every chunk is DECODE and the call
 * degrades to the unpruned one.
 * The prune calls read the bounds, the weights and the zone map on the device and never read the container; they do not synchronise
 * and do not allocate; the survivors' order is the batch's, and no atomic decides a place.  d_tmp: sprintz_mi355x_zone_prune_tmp_bytes(nchunks)
 * bytes of device scratch, aligned to 8 (0 for nchunks == 0).  Classify, the size scan (one launch up to 16 384 chunks, three above) and compact on the stream: three or
 * five launches, none of which counts under a kernel family.
 * Returns, before the device is touched: SPRINTZ_E_INVALID for elem_bytes other than 1 or 2, ndims == 0, chunk_len outside 1..2^30, an
 * unknown mode, a NULL pointer, d_zmin / d_zmax / d_lo / d_hi not aligned to the element size, d_weights not to 4 bytes, d_offsets / d_zlen
 * / d_pos / d_surv_offsets / d_tmp not to 8, and for zone_prune_linear chunk_len % ndims != 0; SPRINTZ_E_UNSUPPORTED for more than 512
 * columns.  nchunks == 0 returns 0 and launches nothing.
 *
 * zone_expand: the compact results of a filter run on (d_comp, d_surv_offsets, n') -- d_cmask [n'][MB], d_ccounts [n'], d_crets [n'], MB =
 * ceil(ceil(chunk_len / ndims) / 8) -- into filter_rows' outputs d_mask [nchunks][MB], d_counts [nchunks], d_rets [nchunks].  A DECODE chunk
 * copies slot d_pos[c] -- but its ret is zlen[c] where zlen[c] < 0, its mask bytes and count then unspecified as in filter_rows: a truncated
 * stream is told by its length alone, and among the survivors a chunk's length runs on over the skipped chunks behind it, so the
 * decoder's own verdict on a chunk the map found damaged is not to be trusted; a NONE chunk gets mask 0, count 0, ret zlen[c]; an ALL chunk the bits of rows r < rows_c set and the rest 0 (the
 * padding bits of its last mask byte included), count rows_c, ret zlen[c].  Every byte of every output is written, each by one writer.
 * d_mask or d_counts may be NULL, not both (then d_cmask / d_ccounts is not read); d_rets is optional (then d_crets is not read); the
 * compact inputs may be NULL where no chunk is DECODE.  One launch, any MB >= 1, any alignment of the masks.
 * Returns, before the device is touched: SPRINTZ_E_INVALID for ndims == 0, chunk_len outside 1..2^30, a NULL d_class / d_pos / d_zlen, both
 * outputs NULL, d_pos / d_zlen / d_crets / d_rets not aligned to 8 bytes, d_ccounts / d_counts not to 4.  nchunks == 0 returns 0 and
 * launches nothing. */
#define SPRINTZ_ZONE_NONE 0u
#define SPRINTZ_ZONE_ALL 1u
#define SPRINTZ_ZONE_DECODE 2u
int sprintz_mi355x_zone_map(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks, uint32_t chunk_len,
                            uint16_t ndims, uint32_t flags, void* d_zmin, void* d_zmax, int64_t* d_zlen, void* hip_stream);
size_t sprintz_mi355x_zone_prune_tmp_bytes(uint64_t nchunks);
int sprintz_mi355x_zone_prune_box(int elem_bytes, uint64_t nchunks, uint32_t chunk_len, uint16_t ndims, const uint64_t* d_offsets,
                                  const void* d_zmin, const void* d_zmax, const int64_t* d_zlen, const void* d_lo, const void* d_hi,
                                  uint32_t mode, uint8_t* d_class, uint64_t* d_pos, uint64_t* d_surv_offsets, void* d_tmp, void* hip_stream);
int sprintz_mi355x_zone_prune_linear(int elem_bytes, uint64_t nchunks, uint32_t chunk_len, uint16_t ndims, const uint64_t* d_offsets,
                                     const void* d_zmin, const void* d_zmax, const int64_t* d_zlen, const int32_t* d_weights, int32_t bias,
                                     int32_t lo, int32_t hi, uint8_t* d_class, uint64_t* d_pos, uint64_t* d_surv_offsets, void* d_tmp,
                                     void* hip_stream);
int sprintz_mi355x_zone_expand(uint64_t nchunks, uint32_t chunk_len, uint16_t ndims, const uint8_t* d_class, const uint64_t* d_pos,
                               const int64_t* d_zlen, const uint8_t* d_cmask, const uint32_t* d_ccounts, const int64_t* d_crets,
                               uint8_t* d_mask, uint32_t* d_counts, int64_t* d_rets, void* hip_stream);
/* Gather rows: N row ranges of a compressed batch, decoded in one launch into a dense [N][rows][ndims] array -- the read
 * the chunked format exists for ("so that queries over arbitrary time intervals are cheap", communicate/intro.tex:55).
 *
 * The batch is given exactly as to sprintz_mi355x_decompress_batch (the payload layout is the one it infers from ndims).
 * With D = ndims and R = chunk_len / D rows a chunk slot, batch row g is row g % R of chunk g / R.  Range i is batch rows
 * [d_starts[i], d_starts[i] + rows); element (row r, column d) of range i lands at d_out[(i*rows + r)*D + d], element type
 * uint8 / uint16, with the value decompress_batch writes for that row under the same options
 * (SPRINTZ_OPT_REF_DECODER_QUIRK included).  Ranges may overlap, repeat, come in any order and span any number of chunks.
 * d_starts lives on the device: the call does not read it on the host, does not synchronise, does not allocate and needs
 * no scratch.  A range costs the decode of every chunk it touches from that chunk's row 0 up to the last row it needs --
 * parsing stops there -- and a chunk shared by several ranges is decoded once per range (sort and merge dense ranges on
 * the caller's side; for single rows named by a mask, sprintz_mi355x_select_rows decodes every chunk once).
 * d_rets (optional, nranges entries): `rows` for a range delivered in full; SPRINTZ_E_INVALID if the range needs a row that
 * does not exist (a chunk >= nchunks, or a row past the rows its chunk's stream holds: the short last chunk);
 * SPRINTZ_E_CORRUPT if a chunk it touches is found damaged before the last row the range needs from it (the smaller code
 * if both).  The rows*D output elements of such a range are unspecified; nothing outside them is written and every
 * other range is exact.  Damage that lies AFTER the last needed row of a chunk may go unnoticed: this call is no integrity
 * check of the container.  When d_rets is given, a small fill kernel runs in front of the decode launch.
 * The container must be laid out as this library writes it (offsets[c+1] - offsets[c] <= compress_bound + alignment).
 * Limit of the fast path (csrc/decode_fast.h; rows of whole 16-byte pieces, a 16-byte aligned d_out): it addresses the container
 * with 32-bit offsets from d_comp.  A stream that ends at d_offsets[c + 1] > 0xfffffff0 - 4096 -- a sub-range of a container larger
 * than 4 GiB addressed from that container's base -- makes every range that touches it SPRINTZ_E_CORRUPT there.  Pass d_comp + base
 * and offsets relative to it instead.  (decompress_batch has no such limit.)
 * Returns, before the device is touched: SPRINTZ_E_INVALID for chunk_len % ndims != 0 (rows must not straddle chunks),
 * rows == 0, chunk_len outside 1..2^30, a NULL d_comp / d_offsets / d_out, a NULL d_starts with nranges > 0, d_out not
 * aligned to the element size, d_starts / d_rets not aligned to 8 bytes; SPRINTZ_E_UNSUPPORTED for more than 512 columns and
 * for the non-RLE codecs.  nranges == 0 returns 0 and launches nothing. */
int sprintz_mi355x_gather_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                               uint32_t chunk_len, uint16_t ndims, const uint64_t* d_starts, uint64_t nranges, uint32_t rows,
                               void* d_out, int64_t* d_rets, void* hip_stream);
/* Select rows: the rows a mask names, decoded and packed densely -- stream compaction fused into the decode.  Every chunk is decoded
 * ONCE, whatever the number of rows it gives (gather_rows decodes a chunk once per range); with filter_rows in front it is
 * "SELECT * WHERE lo <= x <= hi": two decode-speed launches and a prefix sum of the counts between them.
 *
 * The batch is given as to sprintz_mi355x_filter_rows (flags: SPRINTZ_QUERY_GENERAL_LAYOUT and nothing else); chunk_len % ndims == 0
 * is required, as for gather_rows and filter_row_ids.  With D = ndims, R = chunk_len / D and MB = ceil(R / 8):
 *   d_mask : [nchunks][MB] bytes in exactly the layout filter_rows writes -- from filter_rows, from several of its masks combined by
 *            the caller, or from anywhere else: no predicate is evaluated here.  A bit is ignored if its row does not exist: rows
 *            >= R in the last byte, and rows past what the chunk's stream holds (the short last chunk).
 *   d_bases: d_bases[c] is the output row at which chunk c's selected rows start -- normally the exclusive prefix sum of the counts,
 *            computed by the caller.  The bases need not be monotonic: chunks may be placed in any order, with gaps.
 * The i-th set bit of chunk c, in ascending row order over the rows that exist, is row r: its D elements are written to
 * d_out[(d_bases[c] + i)*D ...] -- the values decompress_batch writes for that row under the same options
 * (SPRINTZ_OPT_REF_DECODER_QUIRK included) -- and, if d_ids is not NULL, c*R + r to d_ids[d_bases[c] + i].  A position >= capacity
 * is dropped (compared in 64 bits, before any narrowing); nothing else is written.  Each output row has one writer: no atomics,
 * and the output is deterministic.
 * d_rets (optional) as in decompress_batch: elements decoded, or < 0 for a damaged chunk, of which only the output rows
 * [d_bases[c], d_bases[c] + the set bits of its mask over rows 0 .. R-1) are then unspecified -- nothing is written outside them,
 * and every other chunk is exact.
 * The call does not read the mask or the bases on the host, does not synchronise and does not allocate.  Its launch counts under
 * DEC_FAST (csrc/decode_fast.h: the shapes a filter takes there whose rows are whole 16-byte pieces, (D * elem_bytes) % 16 == 0,
 * with d_out 16-byte aligned and capacity * D * elem_bytes < 0xf0000000) or DEC_GENERIC (csrc/decode_kernel.h, plain 64-bit
 * addresses: everything else, the low-dimension layouts included -- csrc/decode_uni.h is not taught to select).
 * Returns, before the device is touched: SPRINTZ_E_INVALID for chunk_len % ndims != 0, chunk_len outside 1..2^30, an unknown flag,
 * a NULL d_comp / d_offsets / d_mask / d_bases / d_out, d_out not aligned to the element size, d_bases / d_ids / d_rets not aligned
 * to 8 bytes; SPRINTZ_E_UNSUPPORTED for more than 512 columns and for the non-RLE codecs.  nchunks == 0 returns 0 and launches
 * nothing. */
int sprintz_mi355x_select_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                               uint32_t chunk_len, uint16_t ndims, const uint8_t* d_mask, const uint64_t* d_bases,
                               uint64_t capacity, uint32_t flags, void* d_out, uint64_t* d_ids, int64_t* d_rets, void* hip_stream);
/* Aggregate rows: per-window min / max / sum / count of the rows a mask names -- "SELECT count(*), min(x), max(x), sum(x) WHERE ...
 * [GROUP BY time window]" with filter_rows in front, fused into the decode: only the results leave the chip.
 *
 * The batch is given as to sprintz_mi355x_select_rows (flags: SPRINTZ_QUERY_GENERAL_LAYOUT and nothing else; chunk_len % ndims == 0
 * is required).  With D = ndims, R = chunk_len / D, MB = ceil(R / 8), W = window_rows (a multiple of 8, at least 8) and
 * nwin = ceil(R / W): windows are relative to the chunk, exactly as in sprintz_mi355x_query_windows; W >= R gives one aggregate a chunk.
 *   d_mask : [nchunks][MB] bytes in the layout filter_rows writes -- from filter_rows on this batch, from several masks combined, or
 *            from ANOTHER batch on the same time base; no predicate is evaluated here.  A bit is ignored if its row does not exist:
 *            rows >= R in the last byte, rows past what the chunk's stream holds, and a partial last row is not a row.
 * For chunk c, window w and column d the call writes, at index (c*nwin + w)*D + d, over the selected existing rows of that window,
 *   d_min  : the unsigned minimum, element type (uint8 / uint16)    (ops & SPRINTZ_AGG_MIN)
 *   d_max  : the unsigned maximum, element type                     (ops & SPRINTZ_AGG_MAX)
 *   d_sum  : the sum, uint64                                        (ops & SPRINTZ_AGG_SUM)
 * and at index c*nwin + w
 *   d_count: the number of those rows, uint32                       (ops & SPRINTZ_AGG_COUNT)
 * on the values decompress_batch writes under the same options (SPRINTZ_OPT_REF_DECODER_QUIRK included).  A window with no selected
 * row holds the identities: min 0xFF / 0xFFFF, max 0, sum 0, count 0.  Every entry of every selected output is written; an output not
 * selected may be NULL.  One writer an entry, no atomics: the output is deterministic.
 * d_rets (optional) as in query_windows: elements decoded, or < 0 for a damaged chunk, whose own entries are then unspecified --
 * nothing is written outside them, and every other chunk is exact.
 * The call does not read the mask on the host, does not synchronise and does not allocate.  Its launch counts under DEC_FAST
 * (csrc/decode_fast.h: the shapes the windowed query takes there) or DEC_GENERIC (csrc/decode_kernel.h: everything else, the
 * low-dimension layouts included -- csrc/decode_uni.h is not taught the mode).
 * Returns, before the device is touched: SPRINTZ_E_INVALID for chunk_len % ndims != 0, chunk_len outside 1..2^30, a window_rows that
 * is not a multiple of 8 >= 8, ops outside 1..15, a selected output that is NULL, a NULL d_comp / d_offsets / d_mask, d_min / d_max
 * not aligned to the element size, d_count not aligned to 4 bytes, d_sum / d_rets not aligned to 8 bytes, an unknown flag;
 * SPRINTZ_E_UNSUPPORTED for more than 512 columns and for the non-RLE codecs.  nchunks == 0 returns 0 and launches nothing. */
#define SPRINTZ_AGG_MIN 1u
#define SPRINTZ_AGG_MAX 2u
#define SPRINTZ_AGG_SUM 4u
#define SPRINTZ_AGG_COUNT 8u
int sprintz_mi355x_aggregate_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                                  uint32_t chunk_len, uint16_t ndims, const uint8_t* d_mask, uint32_t window_rows, uint32_t ops,
                                  uint32_t flags, void* d_min, void* d_max, uint64_t* d_sum, uint32_t* d_count, int64_t* d_rets,
                                  void* hip_stream);
/* Histogram rows: per-column value counts of the rows a mask names -- the distribution behind "median / p95 / p99 of a channel",
 * "value counts" and "rows per bucket", fused into the decode: only the counts leave the chip.
 *
 * The batch is given as to sprintz_mi355x_aggregate_rows (flags: SPRINTZ_QUERY_GENERAL_LAYOUT and nothing else; chunk_len % ndims == 0
 * is required).  With D = ndims, R = chunk_len / D, MB = ceil(R / 8), W = 8 * elem_bytes:
 *   d_mask : [nchunks][MB] bytes in the layout filter_rows writes, or NULL: every existing row.  A bit is ignored if its row does not
 *            exist: rows >= R in the last byte, rows past what the chunk's stream holds, and a partial last row is not a row.
 *   d_lo   : [D] of element type (uint8 / uint16), or NULL: all zero.
 *   shift, nbins : value x of column d, in a selected row, has t = (x - d_lo[d]) mod 2^W and is counted in bin t >> shift of its column if
 *            that is below nbins; otherwise it is not counted.  0 <= shift < W, 1 <= nbins <= 2^(W - shift).
 *   hist_chunks : H.  Chunks [g*H, (g+1)*H) share histogram g, ngroups = ceil(nchunks / H); 0: the whole batch is one histogram.
 *   d_hist : [ngroups][D][nbins] uint64: entry (g*D + d)*nbins + b is the number of counted samples of column d in bin b among the
 *            chunks of group g, on the values decompress_batch writes under the same options (SPRINTZ_OPT_REF_DECODER_QUIRK included).
 *            The call zeroes it on the stream, then adds: every entry is written and nothing else is.  Integer adds: the result is
 *            exact and the same on every run although atomics are used.
 * One call holds at most SPRINTZ_HIST_MAX_COUNTERS = 16384 counters, D * nbins (a workgroup's table in LDS).  A wider request is split
 * by the caller with d_lo: bins [k*nbins, (k+1)*nbins) of the same shift are one call with d_lo[d] + ((k*nbins) << shift) in place of
 * d_lo[d] -- values outside a call's bins are dropped, so the calls' results lie side by side.  uint8 x 80 columns at full resolution
 * is two calls of 128 bins, d_lo = 0 and d_lo = 128.
 * d_rets (optional) as in aggregate_rows: elements decoded, or < 0 for a damaged chunk, whose own histogram (group) is then
 * unspecified -- nothing is written outside d_hist, and every other group is exact.
 * The call does not read the mask on the host, does not synchronise and does not allocate.  Its launch counts under DEC_FAST
 * (csrc/decode_fast.h: the shapes the windowed query takes there whose table fits the launch's LDS next to the groups' carves) or
 * DEC_GENERIC (csrc/decode_kernel.h: everything else, the low-dimension layouts included -- csrc/decode_uni.h is not taught the mode).
 * A workgroup whose chunks lie in more than one histogram (small H) adds every sample to d_hist directly: correct, and much slower.
 * Returns, before the device is touched: SPRINTZ_E_INVALID for chunk_len % ndims != 0, chunk_len outside 1..2^30, shift >= W, nbins
 * outside 1..2^(W - shift), a NULL d_comp / d_offsets / d_hist, d_hist / d_rets not aligned to 8 bytes, d_lo not aligned to the element
 * size, an unknown flag, more than 2^40 entries of d_hist (ngroups * D * nbins); SPRINTZ_E_UNSUPPORTED for more than 512 columns, for the non-RLE codecs and for D * nbins above
 * SPRINTZ_HIST_MAX_COUNTERS.  nchunks == 0 returns 0 and launches nothing. */
#define SPRINTZ_HIST_MAX_COUNTERS 16384u
int sprintz_mi355x_histogram_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                                  uint32_t chunk_len, uint16_t ndims, const uint8_t* d_mask /* may be NULL */,
                                  const void* d_lo /* may be NULL */, uint32_t shift, uint32_t nbins, uint64_t hist_chunks,
                                  uint32_t flags, uint64_t* d_hist, int64_t* d_rets, void* hip_stream);
/* Moments rows: per-window count, sum, sum of squares and sum of products with one reference column of the rows a mask names -- what
 * variance, standard deviation, covariance and correlation follow from exactly -- fused into the decode: only the results leave the chip.
 *
 * The batch, the flags, the windows and the mask are sprintz_mi355x_aggregate_rows' (chunk_len % ndims == 0 is required; D = ndims,
 * R = chunk_len / D, MB = ceil(R / 8), W = window_rows, a multiple of 8, at least 8, nwin = ceil(R / W): windows are relative to the
 * chunk), except that d_mask may be NULL: every existing row, as in sprintz_mi355x_histogram_rows.  A mask bit is ignored if its row
 * does not exist, and a partial last row is not a row.
 * For chunk c and window w, over the selected existing rows of that window, the call writes
 *   d_count[c*nwin + w]          : the number of those rows, uint32    (ops & SPRINTZ_MOM_COUNT)
 *   d_sum  [(c*nwin + w)*D + d]  : the sum of x_d, uint64              (ops & SPRINTZ_MOM_SUM)
 *   d_sumsq[(c*nwin + w)*D + d]  : the sum of x_d^2, uint64            (ops & SPRINTZ_MOM_SUMSQ)
 *   d_cross[(c*nwin + w)*D + d]  : the sum of x_d * x_ref, uint64      (ops & SPRINTZ_MOM_CROSS; ref = ref_col; for d = ref the sumsq entry)
 * on the unsigned values decompress_batch writes under the same options (SPRINTZ_OPT_REF_DECODER_QUIRK included).  All of them are
 * exact: x * y <= (2^16 - 1)^2 < 2^32, a chunk slot has fewer than 2^30 rows (chunk_len <= 2^30), so every sum of a chunk is below
 * 2^62 and no 64-bit entry wraps.  A window with no selected row holds zeros.  Every entry of every selected output is written, one
 * writer an entry, no atomics: the output is deterministic.  An output not selected may be NULL and is not touched.
 * d_rets (optional) as in aggregate_rows: elements decoded, or < 0 for a damaged chunk, whose own entries are then unspecified --
 * nothing is written outside them, and every other chunk is exact.
 * The call does not read the mask on the host, does not synchronise and does not allocate.  Its launch counts under DEC_FAST
 * (csrc/decode_fast.h: the shapes the windowed query takes there) or DEC_GENERIC (csrc/decode_kernel.h: everything else, the
 * low-dimension layouts included -- csrc/decode_uni.h is not taught the mode).
 * Returns, before the device is touched: SPRINTZ_E_INVALID for chunk_len % ndims != 0, chunk_len outside 1..2^30, a window_rows that
 * is not a multiple of 8 >= 8, ops outside 1..15, a selected output that is NULL, a NULL d_comp / d_offsets, d_count not aligned to
 * 4 bytes, d_sum / d_sumsq / d_cross / d_rets not aligned to 8 bytes, ref_col >= ndims where SPRINTZ_MOM_CROSS is selected (ref_col is
 * ignored otherwise), an unknown flag; SPRINTZ_E_UNSUPPORTED for more than 512 columns and for the non-RLE codecs.  nchunks == 0
 * returns 0 and launches nothing. */
#define SPRINTZ_MOM_COUNT 1u
#define SPRINTZ_MOM_SUM 2u
#define SPRINTZ_MOM_SUMSQ 4u
#define SPRINTZ_MOM_CROSS 8u
int sprintz_mi355x_moments_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                                uint32_t chunk_len, uint16_t ndims, const uint8_t* d_mask /* may be NULL */, uint32_t window_rows,
                                uint32_t ops, uint32_t ref_col, uint32_t flags, uint32_t* d_count, uint64_t* d_sum,
                                uint64_t* d_sumsq, uint64_t* d_cross, int64_t* d_rets, void* hip_stream);
/* Group-by rows: per bin of ONE key column's value, the number of the rows a mask names and their per-column sums -- what conditional
 * means ("mean of every sensor per value of the state channel", a profile plot, a per-class mean where one column is a label) rest on --
 * fused into the decode: only the tables leave the chip.
 *
 * The batch, the flags, the mask and d_rets are sprintz_mi355x_histogram_rows' (flags: SPRINTZ_QUERY_GENERAL_LAYOUT and nothing else;
 * chunk_len % ndims == 0 is required).  With D = ndims, R = chunk_len / D, MB = ceil(R / 8), W = 8 * elem_bytes:
 *   d_mask : [nchunks][MB] bytes in the layout filter_rows writes, or NULL: every existing row.  A bit is ignored if its row does not
 *            exist: rows >= R in the last byte, rows past what the chunk's stream holds, and a partial last row is not a row.
 *   key_col, key_lo, shift, nbins : a selected row whose column key_col holds x has b = ((x - key_lo) mod 2^W) >> shift.  If b >= nbins
 *            the whole row is dropped; otherwise the row belongs to bin b.  key_col < D, key_lo < 2^W, 0 <= shift < W,
 *            1 <= nbins <= 2^(W - shift).
 *   table_chunks : H.  Chunks [t*H, (t+1)*H) share result table t, ntables = ceil(nchunks / H); 0: the whole batch is one table.
 *   d_count[t*nbins + b]          : the number of rows of table t in bin b, uint64                  (ops & SPRINTZ_GBY_COUNT)
 *   d_sum  [(t*nbins + b)*D + d]  : the sum of x_d over those rows, uint64 (the key column's too)   (ops & SPRINTZ_GBY_SUM)
 *            bin-major: the D sums of one bin lie side by side.  The values are those decompress_batch writes under the same options
 *            (SPRINTZ_OPT_REF_DECODER_QUIRK included).  The call zeroes the selected outputs on the stream, then adds: every entry is
 *            written and nothing else is.  Integer adds: the result is exact and the same on every run although atomics are used.  A sum
 *            is below 2^16 * 2^30 * H (values below 2^16, fewer than 2^30 rows a chunk, H chunks a table; the batch's chunks for H = 0):
 *            no 64-bit entry wraps in a table of up to 2^18 chunks of any shape.  An output not selected may be NULL and is not touched.
 * One call holds at most SPRINTZ_GBY_MAX_COUNTERS = 16384 table entries, nbins * (D + 1) (a workgroup's table in LDS).  A wider request
 * is split by the caller with key_lo: bins [k*nbins, (k+1)*nbins) of the same shift are one call with key_lo + ((k*nbins) << shift) in
 * place of key_lo -- rows outside a call's bins are dropped, so the calls' results lie side by side.
 * d_rets (optional) as in histogram_rows: elements decoded, or < 0 for a damaged chunk, whose own table is then unspecified -- nothing
 * is written outside the outputs, and every other table is exact.
 * The call does not read the mask on the host, does not synchronise and does not allocate.  Its launch counts under DEC_FAST
 * (csrc/decode_fast.h: the shapes the windowed query takes there whose table fits the launch's LDS next to the groups' carves) or
 * DEC_GENERIC (csrc/decode_kernel.h: everything else, the low-dimension layouts included -- csrc/decode_uni.h is not taught the mode).
 * A workgroup adds in a table of 32-bit entries, so the table is used only where the rows of a workgroup's chunks times 2^W - 1 fit 32
 * bits.  A workgroup of any other shape, and one whose chunks lie in more than one table (small H), adds every row to d_count / d_sum
 * directly: correct, and much slower.
 * Returns, before the device is touched: SPRINTZ_E_INVALID for chunk_len % ndims != 0, chunk_len outside 1..2^30, key_col >= ndims,
 * key_lo >= 2^W, shift >= W, nbins outside 1..2^(W - shift), ops == 0 or an unknown op bit, a selected output that is NULL, a NULL
 * d_comp / d_offsets, d_count / d_sum / d_rets not aligned to 8 bytes, an unknown flag, more than 2^40 entries of d_sum (ntables *
 * nbins * D); SPRINTZ_E_UNSUPPORTED for more than 512 columns, for the non-RLE codecs and for nbins * (ndims + 1) above
 * SPRINTZ_GBY_MAX_COUNTERS.  nchunks == 0 returns 0 and launches nothing. */
#define SPRINTZ_GBY_COUNT 1u
#define SPRINTZ_GBY_SUM   2u
#define SPRINTZ_GBY_MAX_COUNTERS 16384u      /* nbins * (ndims + 1) */
int sprintz_mi355x_groupby_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                                uint32_t chunk_len, uint16_t ndims, const uint8_t* d_mask /* may be NULL */,
                                uint32_t key_col, uint32_t key_lo, uint32_t shift, uint32_t nbins, uint64_t table_chunks,
                                uint32_t ops, uint32_t flags, uint64_t* d_count, uint64_t* d_sum, int64_t* d_rets, void* hip_stream);
/* Extrema rows: per-window min / max of the rows a mask names WITH the rows they stand in, and the window's first and last selected
 * sample -- "when did the peak happen?", and the M4 reduction a line chart of a long series is drawn from (per pixel column the first,
 * last, minimum and maximum sample, each with its time stamp) -- fused into the decode: only the results leave the chip.
 *
 * The batch, the flags, the windows and the mask are sprintz_mi355x_aggregate_rows' (chunk_len % ndims == 0 is required; D = ndims,
 * R = chunk_len / D, MB = ceil(R / 8), W = window_rows, a multiple of 8, at least 8, nwin = ceil(R / W): windows are relative to the
 * chunk), except that d_mask may be NULL: every existing row, as in sprintz_mi355x_moments_rows.  A mask bit is ignored if its row
 * does not exist, and a partial last row is not a row.
 * For chunk c, window w and column d the call writes, at index (c*nwin + w)*D + d, over the selected existing rows of that window,
 *   d_min   : the unsigned minimum, element type (uint8 / uint16)                         (ops & SPRINTZ_EXT_MIN)
 *   d_max   : the unsigned maximum, element type                                          (ops & SPRINTZ_EXT_MAX)
 *   d_argmin: the chunk-relative row (0 .. R-1, uint32) of the FIRST selected row that holds the minimum   (ops & SPRINTZ_EXT_ARGMIN)
 *   d_argmax: the same for the maximum -- numpy's tie rule                                (ops & SPRINTZ_EXT_ARGMAX)
 *   d_first : column d's value in the window's first selected row, element type          (ops & SPRINTZ_EXT_FIRST)
 *   d_last  : column d's value in the window's last selected row, element type           (ops & SPRINTZ_EXT_LAST)
 * at index (c*nwin + w)*2
 *   d_rows  : the chunk-relative rows of that first and that last selected row, uint32   (ops & SPRINTZ_EXT_ROWS)
 * and at index c*nwin + w
 *   d_count : the number of selected rows, uint32                                         (ops & SPRINTZ_EXT_COUNT)
 * on the values decompress_batch writes under the same options (SPRINTZ_OPT_REF_DECODER_QUIRK included).  A window with no selected
 * row holds min 0xFF / 0xFFFF, max 0, argmin = argmax = both d_rows entries = SPRINTZ_EXT_NO_ROW, first = last = 0, count 0.  Every
 * entry of every selected output is written, one writer an entry, no atomics: the output is deterministic.  An output not selected
 * may be NULL and is not touched; SPRINTZ_EXT_ARGMIN without SPRINTZ_EXT_MIN (and the like) is legal.  Value and row are kept apart
 * in the kernels: window_rows has no upper limit.
 * d_rets (optional) as in aggregate_rows: elements decoded, or < 0 for a damaged chunk, whose own entries are then unspecified --
 * nothing is written outside them, and every other chunk is exact.
 * The call does not read the mask on the host, does not synchronise and does not allocate.  Its launch counts under DEC_FAST
 * (csrc/decode_fast.h: the shapes aggregate_rows takes there) or DEC_GENERIC (csrc/decode_kernel.h: everything else, the
 * low-dimension layouts included -- csrc/decode_uni.h is not taught the mode).
 * Returns, before the device is touched: SPRINTZ_E_INVALID for chunk_len % ndims != 0, chunk_len outside 1..2^30, a window_rows that
 * is not a multiple of 8 >= 8, ops outside 1..255, a selected output that is NULL, a NULL d_comp / d_offsets, a selected d_min / d_max /
 * d_first / d_last not aligned to the element size, a selected d_argmin / d_argmax / d_rows / d_count not aligned to 4 bytes, d_rets
 * not aligned to 8 bytes, an unknown flag; SPRINTZ_E_UNSUPPORTED for more than 512 columns and for the non-RLE codecs.  nchunks == 0
 * returns 0 and launches nothing. */
#define SPRINTZ_EXT_MIN 1u
#define SPRINTZ_EXT_MAX 2u
#define SPRINTZ_EXT_ARGMIN 4u
#define SPRINTZ_EXT_ARGMAX 8u
#define SPRINTZ_EXT_FIRST 16u
#define SPRINTZ_EXT_LAST 32u
#define SPRINTZ_EXT_ROWS 64u
#define SPRINTZ_EXT_COUNT 128u
#define SPRINTZ_EXT_NO_ROW 0xFFFFFFFFu
int sprintz_mi355x_extrema_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                                uint32_t chunk_len, uint16_t ndims, const uint8_t* d_mask /* may be NULL */, uint32_t window_rows, uint32_t ops,
                                uint32_t flags, void* d_min, void* d_max, uint32_t* d_argmin, uint32_t* d_argmax,
                                void* d_first, void* d_last, uint32_t* d_rows, uint32_t* d_count, int64_t* d_rets,
                                void* hip_stream);
/* Segment rows: a row mask's own structure -- per run of selected rows its start, its length and the min / max / sum of every column
 * over it ("for each excursion above the threshold: when did it start, how long did it last, what was the peak and the integral?"), or
 * the same per stretch between two set bits ("for each interval between state changes ...": the change log sprintz_mi355x_filter_linear
 * writes for a state column is that mask) -- fused into the decode: a few bytes a segment leave the chip.
 *
 * The batch, the flags and the mask's layout are sprintz_mi355x_aggregate_rows' (chunk_len % ndims == 0 is required; D = ndims,
 * R = chunk_len / D, MB = ceil(R / 8)); d_mask is required.  rows_c is the number of whole rows chunk c's stream holds, and b[r] is bit
 * r & 7 of d_mask[c*MB + (r >> 3)] for r < rows_c and 0 for every other r: padding bits and the bits of rows the stream does not hold
 * are ignored whatever they contain.  `mode` decides for every row r < rows_c whether it is a MEMBER of a segment and whether it STARTS one:
 *   SPRINTZ_SEG_RUNS  : member = b[r]; start = b[r] && !b[r-1], with b[-1] = 0 -- the segments are the maximal runs of selected rows,
 *                       and the rows between them belong to none
 *   SPRINTZ_SEG_SPLITS: every row is a member; start = b[r] || r == 0 -- the segments tile the chunk's rows, a set bit opens a new one
 * Segment i of chunk c is its i-th start s_i in ascending order and covers rows [s_i, e_i), e_i the first row behind s_i that is not a
 * member or is a start, else rows_c.  Segments are relative to the chunk: one that goes on in the next chunk is two segments here
 * (the second starts at that chunk's row 0).  Its place is p = d_bases[c] + i; a place >= capacity is dropped (compared in 64 bits) and
 * nothing else is written.  The call writes, over the rows of the segment,
 *   d_min  : the unsigned minimum of column d, element type (uint8 / uint16), at p*D + d   (ops & SPRINTZ_SEG_MIN)
 *   d_max  : the unsigned maximum, element type, at p*D + d                                (ops & SPRINTZ_SEG_MAX)
 *   d_sum  : the sum, uint64, at p*D + d                                                   (ops & SPRINTZ_SEG_SUM)
 *   d_rows : e_i - s_i, uint32, at p                                                       (ops & SPRINTZ_SEG_ROWS)
 *   d_start: the batch row c*R + s_i, uint64, at p                                         (ops & SPRINTZ_SEG_START)
 * on the values decompress_batch writes under the same options (SPRINTZ_OPT_REF_DECODER_QUIRK included).  An output not selected may
 * be NULL and is not touched.  Every entry has one writer and there are no atomics: the output is deterministic.  d_bases may come in
 * any order and with gaps; sprintz_mi355x_segment_count gives every chunk's number of segments, of which the caller forms the exclusive
 * prefix sum, as for sprintz_mi355x_select_rows.
 * d_rets (optional) as in aggregate_rows: elements decoded, or < 0 for a damaged chunk.  Of such a chunk only the places
 * [d_bases[c], d_bases[c] + the starts of its mask over rows 0 .. R-1) are unspecified -- nothing is written outside them, and every
 * other chunk is exact.
 * The call does not read the mask on the host, does not synchronise and does not allocate.  Its launch counts under DEC_FAST
 * (csrc/decode_fast.h: the shapes aggregate_rows takes there) or DEC_GENERIC (csrc/decode_kernel.h: everything else, the
 * low-dimension layouts included -- csrc/decode_uni.h is not taught the mode).
 * Returns, before the device is touched: SPRINTZ_E_INVALID for chunk_len % ndims != 0, chunk_len outside 1..2^30, an unknown mode, ops
 * outside 1..31, a selected output that is NULL, a NULL d_comp / d_offsets / d_mask / d_bases, a selected d_min / d_max not aligned to
 * the element size, a selected d_rows not aligned to 4 bytes, a selected d_sum / d_start, d_bases or d_rets not aligned to 8 bytes, an
 * unknown flag; SPRINTZ_E_UNSUPPORTED for more than 512 columns and for the non-RLE codecs.  nchunks == 0 returns 0 and launches nothing. */
#define SPRINTZ_SEG_RUNS   0u
#define SPRINTZ_SEG_SPLITS 1u
#define SPRINTZ_SEG_MIN   1u
#define SPRINTZ_SEG_MAX   2u
#define SPRINTZ_SEG_SUM   4u
#define SPRINTZ_SEG_ROWS  8u
#define SPRINTZ_SEG_START 16u
int sprintz_mi355x_segment_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                                uint32_t chunk_len, uint16_t ndims, const uint8_t* d_mask, uint32_t mode, const uint64_t* d_bases,
                                uint64_t capacity, uint32_t ops, uint32_t flags, void* d_min, void* d_max, uint64_t* d_sum,
                                uint32_t* d_rows, uint64_t* d_start, int64_t* d_rets, void* hip_stream);
/* The segments of every chunk's mask, for sprintz_mi355x_segment_rows' bases: d_counts[c] (uint32) is the number of starts under `mode`
 * among the rows r < rows_c of chunk c.  The call reads the mask alone, never the container: rows_c is R = chunk_len / ndims where d_lens
 * is NULL, and min(R, d_lens[c] / ndims) -- 0 for a negative entry -- where it is given: a chunk's element count as any earlier call's
 * d_rets or sprintz_mi355x_zone_map's d_zlen holds it.  With the true lengths the count is what segment_rows writes for every undamaged
 * chunk.  The mask may start at any address; padding bits and the bits of rows >= rows_c are not trusted.  One launch (it does not count
 * under a SPRINTZ_KF_* family), no synchronisation, no allocation.
 * Returns SPRINTZ_E_INVALID for ndims == 0, chunk_len outside 1..2^30, chunk_len % ndims != 0, an unknown mode, a NULL d_mask / d_counts
 * (with nchunks > 0), d_counts not aligned to 4 bytes or d_lens not aligned to 8.  nchunks == 0 returns 0 and launches nothing. */
int sprintz_mi355x_segment_count(const uint8_t* d_mask, uint64_t nchunks, uint32_t chunk_len, uint16_t ndims, uint32_t mode,
                                 const int64_t* d_lens, uint32_t* d_counts, void* hip_stream);
/* Float rows: the batch decoded straight into scaled float32 / float16 / bfloat16 -- the integer tensor never exists.  The batch is given
 * as to sprintz_mi355x_select_rows (chunk_len % ndims == 0; the RLE codecs; at most 512 columns; a short last chunk may end mid-row).
 * For element e of chunk c, in column d = e % ndims, with x the decoded element:
 *   v   = x, unsigned -- or x sign-extended from 8 / 16 bits with SPRINTZ_FLOAT_SIGNED in flags
 *   z   = fl32(fl32((float)v * d_scale[d]) + d_offset[d])     two IEEE float32 roundings to nearest even, never one fused multiply-add
 *   out = z                                    SPRINTZ_FLOAT_F32
 *       = z rounded to nearest even, binary16  SPRINTZ_FLOAT_F16   (overflow gives +-inf, subnormals are kept)
 *       = z rounded to nearest even, bfloat16  SPRINTZ_FLOAT_BF16  (subnormals are kept)
 * which is, bit for bit, (x.to(float32) * scale + offset).to(dtype) of PyTorch on the CPU.  float32 subnormals are kept too.
 *   d_scale, d_offset: float32 [ndims] on the device.  A NULL d_scale is all 1, a NULL d_offset all 0, with the bits of the explicit arrays.
 *                With finite parameters no NaN can arise; with others the arithmetic is still IEEE float32, and a NaN becomes some quiet NaN.
 *   flags      : SPRINTZ_QUERY_GENERAL_LAYOUT, SPRINTZ_FLOAT_SIGNED and nothing else
 *   d_out      : nchunks * chunk_len elements of the output type; element e of chunk c at d_out[c * chunk_len + e], as decompress_batch places
 *                it, and nothing is written past a chunk's decoded count
 *   d_rets     : (optional) exactly what sprintz_mi355x_decompress_batch writes for the same batch, damaged chunks included
 * One launch (SPRINTZ_KF_DEC_FAST for rows of whole 16-byte pieces, ndims * elem_bytes % 16 == 0, with d_out 16-byte aligned and the other
 * conditions of the plain decode's fast path, counted in OUTPUT bytes; SPRINTZ_KF_DEC_GENERIC otherwise), no synchronisation, no allocation.
 * Returns, before the device is touched: SPRINTZ_E_INVALID for chunk_len % ndims != 0, chunk_len outside 1..2^30, an unknown flag or
 * out_format, a NULL d_comp / d_offsets / d_out, d_out not aligned to the output element size, d_scale / d_offset not aligned to 4 bytes,
 * d_rets not aligned to 8; SPRINTZ_E_UNSUPPORTED for more than 512 columns and for the non-RLE codecs.  nchunks == 0 returns 0 and
 * launches nothing. */
#define SPRINTZ_FLOAT_F32  0
#define SPRINTZ_FLOAT_F16  1
#define SPRINTZ_FLOAT_BF16 2
#define SPRINTZ_FLOAT_SIGNED 2u   /* in flags, next to SPRINTZ_QUERY_GENERAL_LAYOUT */
int sprintz_mi355x_float_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                              uint32_t chunk_len, uint16_t ndims, int out_format, const float* d_scale, const float* d_offset,
                              uint32_t flags, void* d_out, int64_t* d_rets, void* hip_stream);
/* Compress floats: float_rows' way in.  sprintz_mi355x_compress_batch / _compress_batch_dense on a source of float32 / float16 / bfloat16
 * that the encoder quantises while it loads -- the integer tensor never exists.  Element e of the source is in column d = e % ndims
 * (chunk_len % ndims == 0; a short last chunk may end mid-row); for the source element x
 *   v = (float32) x                                           exact for the 16-bit formats
 *   t = fl32(fl32(v - d_offset[d]) * d_inv_scale[d])          two IEEE float32 operations, never contracted into one
 *   r = rint(t), ties to even -- or floor(t) with SPRINTZ_QUANT_FLOOR in flags
 *   q = 0 where r is NaN, else r clamped to [LO, HI]          0 .. 2^W - 1, or -2^(W-1) .. 2^(W-1) - 1 with SPRINTZ_FLOAT_SIGNED (W = 8 elem_bytes)
 * which is, bit for bit, nan_to_num(round_or_floor((x.float() - offset) * inv_scale), nan=0).clamp(LO, HI) of PyTorch on the CPU: +-inf clamp,
 * float32 subnormals are kept.  The encoder takes q as a W-bit two's-complement element, and what the call writes -- streams, d_sizes, d_rets,
 * container and d_offsets -- is byte for byte what sprintz_mi355x_compress_batch / _compress_batch_dense write for the integer tensor q.
 *   d_src      : total_len elements of src_format (SPRINTZ_FLOAT_F32 / _F16 / _BF16), row-major; NO byte outside them is read (the integer
 *                calls' READ_SLACK is not asked for)
 *   d_inv_scale, d_offset: float32 [ndims] on the device; NULL is all 1 / all 0.  inv_scale is the RECIPROCAL of float_rows' scale: with
 *                (1 / scale, offset) this call and float_rows(scale, offset) are each other's way back, within one quantisation step
 *   flags      : SPRINTZ_FLOAT_SIGNED, SPRINTZ_QUANT_FLOOR and nothing else
 *   the other arguments: as sprintz_mi355x_compress_batch / _compress_batch_dense take them (d_tmp: sprintz_mi355x_compress_dense_tmp_bytes)
 * The launch counts under the encoder family that served it: SPRINTZ_KF_ENC_PAIR (5 .. 64 columns with blocks and chunks of whole 16-byte
 * pieces, whatever SPRINTZ_OPT_ENC_PAIR says), _ENC_WIDE / _ENC_SPLIT (65 .. 128 columns), else _ENC_GENERIC -- also for d_src off the 16-byte
 * grid and under SPRINTZ_OPT_NO_FAST; the container under SPRINTZ_KF_DENSE_FUSED or _DENSE_COMPACT.  No synchronisation, no allocation.
 * Measured (profiles/compress_floats.txt; the dense call against torch's quantise expression + compress_batch_dense, ms): headline batch
 * (uint16 x 8) float32 0.909 / 7.72, float16 0.818 / 8.42, bfloat16 0.831 / 8.34; uint8 x 80 at 10 KB chunks 0.794 / 4.91, 0.927 / 5.43,
 * 0.925 / 5.43 -- where the integer call alone takes 0.54 - 0.62 and 0.27.
 * Returns, before the device is touched: SPRINTZ_E_INVALID for chunk_len % ndims != 0, chunk_len outside 1..2^30, an unknown src_format or
 * flag, a NULL d_src / d_slots / d_sizes (or d_dense / d_offsets / d_tmp), d_src not aligned to the source element, d_inv_scale / d_offset
 * not aligned to 4 bytes, and everything sprintz_mi355x_compress_batch refuses; SPRINTZ_E_UNSUPPORTED for more than 512 columns and for the
 * non-RLE codecs.  Every message names the call.  total_len == 0 returns 0, launches nothing and writes nothing. */
#define SPRINTZ_QUANT_FLOOR 4u   /* in flags, next to SPRINTZ_FLOAT_SIGNED */
int sprintz_mi355x_compress_batch_float(int codec, int elem_bytes, const void* d_src, int src_format, const float* d_inv_scale,
                                        const float* d_offset, uint32_t flags, uint64_t total_len, uint32_t chunk_len, uint16_t ndims,
                                        void* d_slots, size_t slot_stride, uint32_t* d_sizes, int64_t* d_rets, void* hip_stream);
int sprintz_mi355x_compress_batch_float_dense(int codec, int elem_bytes, const void* d_src, int src_format, const float* d_inv_scale,
                                              const float* d_offset, uint32_t flags, uint64_t total_len, uint32_t chunk_len, uint16_t ndims,
                                              void* d_slots, size_t slot_stride, uint32_t* d_sizes, int64_t* d_rets, void* d_dense,
                                              uint64_t* d_offsets, void* d_tmp, void* hip_stream);
/* Rolling rows: per element, its column's minimum / maximum / sum over the window_rows rows that END at its row -- pandas' rolling(W,
 * min_periods=1) -- straight from the compressed batch; the decoded tensor never exists.  The batch is given as to
 * sprintz_mi355x_select_rows (chunk_len % ndims == 0; the RLE codecs; at most 512 columns; a short last chunk may end mid-row).  The batch's
 * rows are g = 0 .. G - 1, row g being row g % R of chunk g / R, R = chunk_len / ndims.  For every element that exists, in row g and column d:
 *   out[g, d] = op(x[max(0, g - W + 1) .. g, d])          a trailing window, clipped at the batch's first row
 * with op the unsigned minimum / maximum in the element type (d_min, d_max) or the sum as an int32 (d_sum), placed where decompress_batch
 * places the element: element e of chunk c at out[c * chunk_len + e]; nothing is written past a chunk's decoded count.  A mean is the sum
 * divided by the row's count min(g + 1, W).
 *   window_rows: W, a multiple of 8 with 8 <= W <= R (one predecessor chunk suffices at a seam) and W * (2^(8 elem_bytes) - 1) < 2^31.
 *                A chunk's last W + 8 rows wait in LDS: where the rings of the chunks a workgroup decodes do not fit its 160 KB, the call
 *                returns SPRINTZ_E_UNSUPPORTED and sprintz_mi355x_last_error names the largest window_rows the shape allows.
 *   ops        : a non-empty OR of SPRINTZ_ROLL_MIN / _MAX / _SUM; an output must be given exactly where its op is
 *   flags      : SPRINTZ_QUERY_GENERAL_LAYOUT and nothing else
 *   d_tmp      : with nchunks > 1, scratch of nchunks * stride bytes, 16-byte aligned, stride = (16 + (W - 1) * ndims * elem_bytes + 15) & ~15
 *                (roll_tmp_stride in geom.h): a chunk leaves its element count and its last W - 1 rows there.  Its content before the call
 *                does not matter.  Ignored (may be NULL) with one chunk.
 *   d_rets     : (optional) exactly what sprintz_mi355x_decompress_batch writes for the same batch, damaged chunks included
 * Two launches on the stream -- the decode (SPRINTZ_KF_DEC_FAST for rows of whole 16-byte pieces of 8 .. 64 columns with every output 16-byte aligned,
 * while the rings fit its LDS budget; SPRINTZ_KF_DEC_GENERIC otherwise), in which a chunk is its own beginning, and with
 * nchunks > 1 a seam pass that takes the last rows of the chunk in front into the windows of each chunk's first W - 1 rows -- no
 * synchronisation, no allocation.  A chunk behind a damaged one keeps its chunk-local windows: exact from its row W - 1 on.
 * Returns, before the device is touched: SPRINTZ_E_INVALID for chunk_len % ndims != 0, chunk_len outside 1..2^30, an unknown flag, a
 * window_rows that is no multiple of 8, below 8, above R or too large for the int32 sum, ops outside 1..7, an op without its output or an
 * output without its op, d_min / d_max not aligned to the element size, d_sum to 4 bytes, d_rets to 8, d_tmp missing or not aligned to 16
 * with nchunks > 1; SPRINTZ_E_UNSUPPORTED for more than 512 columns, the non-RLE codecs and a window beyond the LDS bound.  nchunks == 0
 * returns 0 and launches nothing. */
#define SPRINTZ_ROLL_MIN 1u
#define SPRINTZ_ROLL_MAX 2u
#define SPRINTZ_ROLL_SUM 4u
int sprintz_mi355x_rolling_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                                uint32_t chunk_len, uint16_t ndims, uint32_t window_rows, uint32_t ops, uint32_t flags,
                                void* d_min, void* d_max, int32_t* d_sum, void* d_tmp, int64_t* d_rets, void* hip_stream);
/* Project rows: SELECT a, b -- the batch decoded into a dense [rows, ncolumns] tensor of the columns a slot table names, in the element type or
 * as float_rows converts; the other columns are decoded (the predictors need them) and never stored.  The batch is given as to
 * sprintz_mi355x_select_rows (chunk_len % ndims == 0; the RLE codecs; at most 512 columns; a short last chunk may end mid-row).  The batch's
 * rows are g = 0 .. G - 1, row g being row g % R of chunk g / R, R = chunk_len / ndims; chunk c's rows start at output row c * R.  For every
 * element that exists, in row g and column d with s = d_slots[d] in 0 .. ncolumns - 1:
 *   out[g * ncolumns + s] = x[g, d]                                          format SPRINTZ_PROJECT_RAW, in the element type
 *                         = float_rows' value with d_scale[s], d_offset[s]    format SPRINTZ_PROJECT_F32 / _F16 / _BF16, bit for bit float_rows' rule
 *   d_slots    : int32 [ndims] on the device: column d's slot in an output row, or -1 for a column that is not wanted.  ANY entry outside
 *                0 .. ncolumns - 1 is read as "not wanted": a damaged table can misplace values inside d_out and never writes outside it.  Two
 *                columns with one slot leave one of their values there.  A slot no column names is not written.
 *   ncolumns   : K, 1 .. ndims
 *   format     : SPRINTZ_PROJECT_RAW (0), or 1 + a SPRINTZ_FLOAT_* format
 *   d_scale, d_offset: float32 [ncolumns] on the device, indexed by SLOT; NULL is all 1 / all 0.  Only with a float format.
 *   flags      : SPRINTZ_QUERY_GENERAL_LAYOUT, SPRINTZ_FLOAT_SIGNED (a float format alone) and nothing else
 *   d_out      : nchunks * R * ncolumns elements of the output type (a chunk slot each chunk, as for every batch call: a damaged stream may
 *                decode to more rows than its chunk had, never to more than R); the first G * ncolumns of them are the result, G the rows
 *                the batch decodes to.  Nothing is written past a chunk's decoded count: where the batch ends mid-row the elements of that
 *                row that do not exist are not written.  (SPRINTZ_KF_DEC_FAST reaches the chunks of a wavefront with
 *                32-bit offsets, as for float_rows: where 4096 projected chunk slots, R * ncolumns output elements each, pass 0xf0000000
 *                bytes the generic kernel runs.)
 *   d_rets     : (optional) exactly what sprintz_mi355x_decompress_batch writes for the same batch -- a chunk's count of ALL its elements --
 *                damaged chunks included
 * One launch (SPRINTZ_KF_DEC_FAST for 3 .. 64 columns where the plain decode runs there and the projected block, 8 * ncolumns * elem_bytes, is a
 * whole number of 16-byte pieces, with d_out 16-byte aligned; SPRINTZ_KF_DEC_GENERIC otherwise), no synchronisation, no allocation.
 * Returns, before the device is touched: SPRINTZ_E_INVALID for ncolumns == 0 or above ndims, chunk_len % ndims != 0, chunk_len outside
 * 1..2^30, an unknown flag or format, d_scale / d_offset / SPRINTZ_FLOAT_SIGNED with SPRINTZ_PROJECT_RAW, a NULL d_comp / d_offsets / d_slots /
 * d_out, d_out not aligned to the output element size, d_slots / d_scale / d_offset not aligned to 4 bytes, d_rets to 8;
 * SPRINTZ_E_UNSUPPORTED for more than 512 columns and for the non-RLE codecs.  nchunks == 0 returns 0 and launches nothing. */
#define SPRINTZ_PROJECT_RAW  0
#define SPRINTZ_PROJECT_F32  1   /* 1 + SPRINTZ_FLOAT_F32 */
#define SPRINTZ_PROJECT_F16  2
#define SPRINTZ_PROJECT_BF16 3
int sprintz_mi355x_project_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                                uint32_t chunk_len, uint32_t ndims, const int32_t* d_slots, uint32_t ncolumns, int format,
                                const float* d_scale, const float* d_offset, uint32_t flags, void* d_out, int64_t* d_rets, void* hip_stream);
/* Cumulative rows: per element, its column's running minimum / maximum / sum from the batch's first row to its own row -- cummin, cummax and cumsum
 * (the expanding window; pandas' expanding()) -- straight from the compressed batch; the decoded tensor never exists.  The batch is given as to
 * sprintz_mi355x_rolling_rows (chunk_len % ndims == 0; the RLE codecs; at most 512 columns; a short last chunk may end mid-row: a column has the
 * rows it has).  The batch's rows are g = 0 .. G - 1, row g being row g % R of chunk g / R, R = chunk_len / ndims.  For every element that exists,
 * in row g and column d:
 *   min[g, d] = min(seed_min[d], x[0 .. g, d])        unsigned, in the element type
 *   max[g, d] = max(seed_max[d], x[0 .. g, d])        unsigned, in the element type
 *   sum[g, d] = seed_sum[d] + sum(x[0 .. g, d])       modulo 2^64, stored as an int64 (sum_bytes 8) or its low 32 bits as an int32 (sum_bytes 4)
 * placed where decompress_batch places the element: element e of chunk c at out[c * chunk_len + e]; nothing is written past a chunk's decoded
 * count.  The samples are the ones sprintz_mi355x_decompress_batch writes under the same options, SPRINTZ_OPT_REF_DECODER_QUIRK included.  An
 * expanding mean is the sum divided by the rows so far, g + 1.
 *   ops        : a non-empty OR of SPRINTZ_CUM_MIN / _MAX / _SUM; an output must be given exactly where its op is
 *   sum_bytes  : 4 or 8, the bytes of an element of d_sum (checked whatever ops holds)
 *   flags      : SPRINTZ_QUERY_GENERAL_LAYOUT and nothing else
 *   d_carry_in : (optional) the seeds, uint64 [3 * ndims]: a min row, a max row and a sum row.  The min and the max seeds are read modulo 2^(8
 *                elem_bytes).  NULL: the identities -- all ones of the element type, 0 and 0.
 *   d_carry_out: (optional) the same layout: the state behind the batch's last element of each column.  carry_out of one call, given as carry_in
 *                to the next, yields exactly the cumulative of the concatenated batches: this is how a stream longer than one batch, or one rank's
 *                share of it, is continued.  The row of an op that was not asked for is its seed, passed through.  It may be the buffer d_carry_in is.
 *   d_tmp      : with nchunks > 1, scratch of sprintz_mi355x_cumulative_tmp_bytes(nchunks, ndims) bytes, 16-byte aligned (36 bytes a chunk and
 *                column, 8 a chunk, and rounding: the chunks' entering states, and the totals they are made from).  Its content before the call does
 *                not matter.  Ignored (may be NULL) with nchunks <= 1, for which cumulative_tmp_bytes returns 0.
 *   d_rets     : (optional) exactly what sprintz_mi355x_decompress_batch writes for the same batch, damaged chunks included
 * A damaged chunk (d_rets < 0) contributes the identity to everything behind it and to d_carry_out: the chunks behind it continue from the state
 * in front of it.  Its own slot of the outputs is unspecified; nothing outside that slot is touched.
 * With nchunks > 1, three launches on the stream, none of which waits for a workgroup of its own or of another launch: the totals (the windowed
 * query with one window a chunk: every chunk's min / max / sum and return value into d_tmp), the scan (a workgroup a column walks the chunks and
 * leaves each chunk's entering state, seeded with d_carry_in; it writes d_carry_out) and the decode (SPRINTZ_KF_DEC_FAST for rows of whole 16-byte
 * pieces of 8 .. 64 columns with every output 16-byte aligned; SPRINTZ_KF_DEC_GENERIC otherwise), in which a lane keeps the running values of its
 * column in registers.  With one chunk the decode alone, which reads d_carry_in and writes d_carry_out itself.  nchunks == 0 launches nothing, or,
 * with d_carry_out given, one tiny kernel that copies the seeds there.  No synchronisation, no allocation.
 * Returns, before the device is touched: SPRINTZ_E_INVALID for chunk_len % ndims != 0, chunk_len outside 1..2^30, an unknown flag, ops outside
 * 1..7, an op without its output or an output without its op, sum_bytes other than 4 or 8, d_min / d_max not aligned to the element size, d_sum
 * to sum_bytes, d_carry_in / d_carry_out / d_rets to 8, d_tmp to 16, d_tmp missing with nchunks > 1; SPRINTZ_E_UNSUPPORTED for more than 512
 * columns and for the non-RLE codecs. */
#define SPRINTZ_CUM_MIN 1u
#define SPRINTZ_CUM_MAX 2u
#define SPRINTZ_CUM_SUM 4u
size_t sprintz_mi355x_cumulative_tmp_bytes(uint64_t nchunks, uint16_t ndims);
int sprintz_mi355x_cumulative_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                                   uint32_t chunk_len, uint16_t ndims, uint32_t ops, int sum_bytes /* 4 or 8 */, uint32_t flags,
                                   void* d_min, void* d_max, void* d_sum, const uint64_t* d_carry_in, uint64_t* d_carry_out,
                                   void* d_tmp, int64_t* d_rets, void* hip_stream);
/* Derive rows: SELECT <expression> -- K linear forms of every row and of the row in front of it, straight from the compressed batch; the decoded
 * tensor never exists.  This is sprintz_mi355x_filter_linear's sum itself, K of them a row, returned instead of tested: the spread of two columns
 * (a - b), the sum of a few, a column minus twice its neighbour, or, with lag weights, numpy.diff / pandas' diff().  The batch is given as to
 * sprintz_mi355x_filter_linear (chunk_len % ndims == 0; the RLE codecs; at most 512 columns; a short last chunk may end mid-row: only whole rows are
 * rows).  The batch's rows are g = 0 .. G - 1, row g being row g % R of chunk g / R, R = chunk_len / ndims.  For 1 <= nforms <= 16 and every row g:
 *   s[g, k] = d_bias[k] + sum_d d_weights[k][d] x[g, d] + sum_d d_lag_weights[k][d] x[p(g), d]      modulo 2^32, read as an int32
 * with x the unsigned sample, p(g) = g - 1 and p(0) = 0 -- row 0 is its own predecessor (numpy.diff(prepend = x[0])) -- unless d_prev gives the row
 * in front of row 0: ndims elements of the element type, the last row of the batch before this one, so that a stream continued over batches
 * differentiates exactly.  d_lag_weights == NULL: no lag term, no scratch, no second launch, and d_prev is ignored.  s is exact wherever
 * |bias| + sum (|w| + |u|) (2^(8 elem_bytes) - 1) < 2^31 (the bound the Python layer refuses by); beyond it the value is the wrapped one.
 * Output: a dense [G, nforms] tensor, row g at element g * nforms; a chunk's rows start at element c * R * nforms; rows that do not exist are not
 * written.
 *   format   : SPRINTZ_DERIVE_I32: out[g * nforms + k] = s[g, k], an int32
 *              SPRINTZ_DERIVE_F32 / _F16 / _BF16: z = fl32(fl32((float)s * d_scale[k]) + d_offset[k]) -- the int32 -> float32 conversion rounds to
 *              nearest even (from |s| >= 2^24 on), the two float32 operations are never one fma -- stored as float32, or rounded to nearest even to
 *              float16 / bfloat16 as float_rows rounds: bit for bit torch's CPU (s.to(float32) * scale + offset).to(dtype)
 *   d_scale, d_offset : float32 [nforms], or NULL: all 1 / all 0; with a float format only
 *   flags    : SPRINTZ_QUERY_GENERAL_LAYOUT and nothing else
 *   d_tmp    : with d_lag_weights, scratch of sprintz_mi355x_derive_rows_tmp_bytes(elem_bytes, nchunks, ndims) bytes, 8-byte aligned (the first and the
 *              last row of every chunk; filter_linear's layout and size).  Its content before the call does not matter.
 *   d_rets   : (optional) exactly what sprintz_mi355x_decompress_batch writes for the same batch, damaged chunks included
 * A damaged chunk (d_rets < 0): its own rows are unspecified, and so is row 0 of the chunk behind it where a lag term is given; every other row is
 * exact, and nothing outside the batch's chunk slots is written.
 * One launch (SPRINTZ_KF_DEC_FAST on the one-column-a-lane mappings, up to 64 columns, for the shapes the plain decode takes there with a 16-byte
 * aligned d_out; SPRINTZ_KF_DEC_GENERIC otherwise); with a lag term and more than one chunk, or d_prev, a second small one behind it on the stream that
 * writes row 0 of the chunks again with their true predecessors.  nchunks == 0 returns 0 and launches nothing.  No synchronisation, no allocation.
 * Returns, before the device is touched: SPRINTZ_E_INVALID for a NULL d_comp / d_offsets / d_weights / d_out, nforms outside 1..16, chunk_len %
 * ndims != 0, chunk_len outside 1..2^30, an unknown format or flag, d_scale / d_offset with SPRINTZ_DERIVE_I32, d_out not aligned to the output
 * element, d_weights / d_lag_weights / d_bias / d_scale / d_offset not aligned to 4, d_prev to the element size, d_rets to 8, d_tmp NULL or not
 * aligned to 8 with d_lag_weights; SPRINTZ_E_UNSUPPORTED for more than 512 columns and for the non-RLE codecs. */
#define SPRINTZ_DERIVE_I32  0
#define SPRINTZ_DERIVE_F32  1   /* 1 + SPRINTZ_FLOAT_F32 */
#define SPRINTZ_DERIVE_F16  2
#define SPRINTZ_DERIVE_BF16 3
uint64_t sprintz_mi355x_derive_rows_tmp_bytes(int elem_bytes, uint64_t nchunks, uint16_t ndims);
int sprintz_mi355x_derive_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                               uint32_t chunk_len, uint16_t ndims, uint32_t nforms,
                               const int32_t* d_weights,      /* [nforms][ndims] */
                               const int32_t* d_lag_weights,  /* [nforms][ndims] or NULL */
                               const int32_t* d_bias,         /* [nforms] or NULL: all 0 */
                               int format,                    /* SPRINTZ_DERIVE_I32 0, _F32 1, _F16 2, _BF16 3 */
                               const float* d_scale, const float* d_offset,   /* [nforms], float formats only */
                               const void* d_prev,            /* [ndims] element type, or NULL */
                               uint32_t flags, void* d_tmp, void* d_out, int64_t* d_rets, void* hip_stream);
/* FIR rows: a per-column tap filter over the rows -- a weighted history of every column, straight from the compressed batch; the decoded tensor never
 * exists.  Where sprintz_mi355x_rolling_rows looks back W rows with weights of one and sprintz_mi355x_derive_rows weighs the one row in front, this
 * takes ntaps integer weights a column: a smoothing filter (binomial, triangular taps), the k-row difference x[g] - x[g - k] (pandas' diff(periods=k)),
 * shift(k), a second difference, a band-pass or differentiator kernel, a matched filter against a short template.  The batch is given as to
 * sprintz_mi355x_rolling_rows (chunk_len % ndims == 0; the RLE codecs; at most 512 columns; a short last chunk may end mid-row).  The batch's rows are
 * g = 0 .. G - 1, row g being row g % R of chunk g / R, R = chunk_len / ndims.  For T = ntaps, 1 <= T <= 256 with T - 1 <= R, and every element that
 * exists, in row g and column d:
 *   y[g, d] = d_bias[d] + sum_{j = 0 .. T - 1} d_taps[j][d] x[g - j, d]          modulo 2^32, read as an int32
 * with x the unsigned sample; d_taps[0] weighs the row itself.  Rows in front of row 0 come from d_prev: [T - 1][ndims] of the element type, the last
 * rows of the batch before this one, its last row being row -1 -- a stream continued over batches then filters exactly.  d_prev == NULL: rows in front
 * of row 0 equal row 0 (edge replication: derive_rows' "row 0 is its own predecessor"; a smoothing filter has no start-up transient).  The zero
 * initial state of scipy.signal.lfilter is a d_prev of zeros.  y is exact wherever |bias[d]| + sum_j |taps[j][d]| (2^(8 elem_bytes) - 1) < 2^31 (the
 * bound the Python layer refuses by); beyond it the value is the wrapped one.
 * Output: every element at its own place, element e of chunk c at d_out[c * chunk_len + e], as rolling_rows places its results -- for whole-row
 * batches a dense [G, ndims] view; elements that do not exist are not written.
 *   format   : SPRINTZ_DERIVE_I32: the int32 y; SPRINTZ_DERIVE_F32 / _F16 / _BF16: fl32(fl32((float)y * d_scale[d]) + d_offset[d]), converted and
 *              rounded exactly as derive_rows converts: bit for bit torch's CPU (y.to(float32) * scale + offset).to(dtype)
 *   d_scale, d_offset : float32 [ndims], or NULL: all 1 / all 0; with a float format only
 *   flags    : SPRINTZ_QUERY_GENERAL_LAYOUT and nothing else
 *   d_tmp    : with ntaps > 1, scratch of sprintz_mi355x_fir_rows_tmp_bytes(elem_bytes, nchunks, ndims, ntaps) bytes, 16-byte aligned: per chunk a
 *              16-byte head (the elements the chunk decoded to; 0: damaged), its first T - 1 raw rows, then its last T - 1 raw rows, the stride
 *              rounded up to 16 (fir_tmp_stride in geom.h).  Its content before the call does not matter.  ntaps == 1: no scratch, no second launch,
 *              and d_prev is ignored.
 *   d_rets   : (optional) exactly what sprintz_mi355x_decompress_batch writes for the same batch, damaged chunks included
 * A chunk's last Wh + 8 raw rows, Wh = T - 1 rounded up to a multiple of 8, wait in LDS (rolling_rows' ring): where the rings of the chunks a
 * workgroup decodes do not fit its 160 KB, the call returns SPRINTZ_E_UNSUPPORTED and sprintz_mi355x_last_error names the largest ntaps the shape takes.
 * A damaged chunk (d_rets < 0): its own rows are unspecified, and so are the first T - 1 rows of the chunk behind it; every other row is exact, and
 * nothing outside the batch's chunk slots or outside the scratch is written.
 * Two launches on the stream -- the decode (SPRINTZ_KF_DEC_FAST for rows of whole 16-byte pieces of 8 .. 64 columns with a 16-byte aligned d_out, while
 * rings and taps fit its LDS budget; SPRINTZ_KF_DEC_GENERIC otherwise), in which rows in front of a chunk's first contribute nothing, and with ntaps > 1
 * a seam pass that computes the first T - 1 rows of every chunk again from raw rows -- no synchronisation, no allocation.  nchunks == 0 returns 0 and
 * launches nothing.
 * Returns, before the device is touched: SPRINTZ_E_INVALID for a NULL d_comp / d_offsets / d_taps / d_out, ntaps outside 1..256, ntaps - 1 >
 * chunk_len / ndims, chunk_len % ndims != 0, chunk_len outside 1..2^30, an unknown format or flag, d_scale / d_offset with SPRINTZ_DERIVE_I32, d_out not
 * aligned to the output element, d_taps / d_bias / d_scale / d_offset not aligned to 4, d_prev to the element size, d_rets to 8, d_tmp NULL or not
 * aligned to 16 with ntaps > 1; SPRINTZ_E_UNSUPPORTED for more than 512 columns, the non-RLE codecs and a history beyond the LDS bound. */
uint64_t sprintz_mi355x_fir_rows_tmp_bytes(int elem_bytes, uint64_t nchunks, uint16_t ndims, uint32_t ntaps);
int sprintz_mi355x_fir_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks,
                            uint32_t chunk_len, uint16_t ndims, uint32_t ntaps,
                            const int32_t* d_taps,   /* [ntaps][ndims] */
                            const int32_t* d_bias,   /* [ndims] or NULL: all 0 */
                            int format,              /* SPRINTZ_DERIVE_I32 / _F32 / _F16 / _BF16 */
                            const float* d_scale, const float* d_offset,   /* [ndims], float formats only */
                            const void* d_prev,      /* [ntaps - 1][ndims] element type, or NULL */
                            uint32_t flags, void* d_tmp, void* d_out, int64_t* d_rets, void* hip_stream);
/* single-call forms over host buffers; result: ndims uint64 (may be NULL);
 * return value as decompress (elements), < 0 on error */
int64_t sprintz_mi355x_query_delta_8b(const int8_t* src, uint8_t* dest, int op, int materialize, uint32_t flags, uint64_t* result);
int64_t sprintz_mi355x_query_delta_16b(const int16_t* src, uint16_t* dest, int op, int materialize, uint32_t flags, uint64_t* result);
int64_t sprintz_mi355x_query_xff_8b(const int8_t* src, uint8_t* dest, int op, int materialize, uint32_t flags, uint64_t* result);
int64_t sprintz_mi355x_query_xff_16b(const int16_t* src, uint16_t* dest, int op, int materialize, uint32_t flags, uint64_t* result);

/* single-call forms of the non-RLE codecs over host buffers; replace
 *   compress_rowmajor_{8b,16b} / decompress_rowmajor_{8b,16b}                cpp/Compress/sprintz_delta.h:26-31,63-66
 *   compress_rowmajor_delta_{8b,16b} / decompress_rowmajor_delta_{8b,16b}    cpp/Compress/sprintz_delta.h:37-42,72-76
 *   compress8b_rowmajor_xff / decompress8b_rowmajor_xff                      cpp/Compress/sprintz_xff.h:28-31
 * codec: SPRINTZ_CODEC_DELTA_NORLE, SPRINTZ_CODEC_BITPACK_NORLE or SPRINTZ_CODEC_XFF_NORLE; return values in elements as above */
int64_t sprintz_mi355x_compress_norle(int codec, int elem_bytes, const void* src, uint32_t len, void* dest, uint16_t ndims);
int64_t sprintz_mi355x_decompress_norle(int codec, int elem_bytes, const void* src, void* dest);

/* ------------------------------------------------------------------------
 * Huff0 wire format, both directions.  The paper's entropy stage is Yann Collet's
 * Huff0 (communicate/ubicomp/method.tex:293-297), a third-party coder the
 * reference neither vendors nor pins; this entry point decodes GENUINE Huff0
 * blocks -- what HUF_compress of zstd 1.4.x / lzbench's huff0 writes: tree
 * description (4-bit or FSE-compressed weights), 3 x u16 jump table, 4 bit
 * streams -- one block per chunk, so that a container entropy-coded by that
 * library can be taken straight to sprintz_mi355x_decompress_batch.  Replaces
 * HUF_decompress(dst, dstSize, cSrc, cSrcSize) per chunk, with its conventions:
 * block bytes == decoded bytes means stored, 1 byte means one repeated byte.
 *   d_blocks + d_block_offsets[c] .. [c+1] : chunk c's block
 *   d_out + d_out_offsets[c] .. [c+1]      : where its bytes go (the sizes are
 *                                            the caller's, as with HUF_decompress)
 *   d_rets[c] (optional): decoded bytes, or SPRINTZ_E_CORRUPT for a damaged block
 *   (nothing is read or written outside the chunk's two ranges).
 * d_blocks must be 16-byte aligned and readable 16 bytes past its end.  Format restated in
 * oracle/huf0_oracle.c; kernel in sprintz_amd/csrc/huf0.hip.
 * ---------------------------------------------------------------------- */
int sprintz_mi355x_huf0_decompress_batch(const void* d_blocks, const uint64_t* d_block_offsets, uint64_t nchunks, void* d_out,
                                         const uint64_t* d_out_offsets, int64_t* d_rets, void* hip_stream);
/* The same with the caller's workspace (d_tmp: sprintz_mi355x_huf0_decode_tmp_bytes(nchunks) bytes, 16-byte aligned;
 * holds one 320-byte code descriptor per chunk and two flag arrays between the launches).  The form above allocates it
 * stream-ordered (hipMallocAsync) per call; a caller with a steady batch size passes its own.  A block's
 * streams are limited to 128 MiB each (HUF_compress never writes a block above 128 KB). */
size_t sprintz_mi355x_huf0_decode_tmp_bytes(uint64_t nchunks);
int sprintz_mi355x_huf0_decompress_batch_ws(const void* d_blocks, const uint64_t* d_block_offsets, uint64_t nchunks, void* d_out,
                                            const uint64_t* d_out_offsets, int64_t* d_rets, void* d_tmp, void* hip_stream);
/* The same with a HINT: max_block_bytes = an upper bound of the batch's block sizes (0 = unknown).  Small batches
 * (SPRINTZ_OPT_HUF0_SYNC_CHUNKS) keep a chunk's whole block in LDS; the hint sizes that image (up to 16 KB a block; without one 4 KB).
 * A block above the image -- or above a wrong hint -- is still decoded, from global memory: the hint is never trusted for safety. */
int sprintz_mi355x_huf0_decompress_batch_hint(const void* d_blocks, const uint64_t* d_block_offsets, uint64_t nchunks, void* d_out,
                                              const uint64_t* d_out_offsets, int64_t* d_rets, void* d_tmp, uint32_t max_block_bytes,
                                              void* hip_stream);
/* The other direction: container (d_dense, d_offsets[nchunks+1], d_sizes[nchunks] = exact stream bytes, as
 * sprintz_mi355x_compact leaves them) -> one Huff0 block per chunk, byte-dense at d_blocks +
 * d_block_offsets[c] (d_block_offsets[nchunks] = total), each one a block HUF_decompress(dst, size of
 * the chunk, block, size of the block) decodes -- the write side of lzbench's huff0 stage.  The
 * format leaves the encoder free; what is written is specified by oracle/huf0_oracle.c
 * (oracle_huf0_compress_batch: one code table per 64 chunks repeated in every block, FSE-coded or 4-bit
 * weights, stored / one-byte blocks under HUF_decompress's conventions) and the kernels are
 * byte-exact with it.  d_blocks: sprintz_mi355x_huf0_bound(sum of sizes, nchunks) bytes; d_tmp:
 * sprintz_mi355x_huf0_tmp_bytes(nchunks). */
size_t sprintz_mi355x_huf0_tmp_bytes(uint64_t nchunks);
size_t sprintz_mi355x_huf0_bound(uint64_t total_stream_bytes, uint64_t nchunks);
int sprintz_mi355x_huf0_compress_batch(const void* d_dense, const uint64_t* d_offsets, const uint32_t* d_sizes, uint64_t nchunks,
                                       void* d_blocks, uint64_t* d_block_offsets, void* d_tmp, void* hip_stream);
/* The same direction, with one code table per chunk: each block is byte for byte what libzstd 1.4.8's
 * HUF_compress2(dst, HUF_compressBound(size), chunk, size, 255, table_log) returns -- the bytes the paper's
 * CPU pipeline writes (a chunk HUF_compress declines is stored verbatim, a chunk of one repeated byte is that
 * byte, an empty chunk an empty block).  table_log: 0 (= 11, plain HUF_compress) or 5 .. 12.  Specification:
 * tests/huf0_exact_model.py; kernels in sprintz_amd/csrc/huf0_exact.h.  d_blocks: sprintz_mi355x_huf0_bound(sum
 * of sizes, nchunks) bytes (a block is never larger than its chunk); d_tmp: sprintz_mi355x_huf0_exact_tmp_bytes(nchunks). */
size_t sprintz_mi355x_huf0_exact_tmp_bytes(uint64_t nchunks);
int sprintz_mi355x_huf0_compress_batch_exact(const void* d_dense, const uint64_t* d_offsets, const uint32_t* d_sizes, uint64_t nchunks,
                                             unsigned table_log /* 0 = 11; 5..12 */, void* d_blocks, uint64_t* d_block_offsets,
                                             void* d_tmp, void* hip_stream);

/* ------------------------------------------------------------------------
 * Stand-alone transforms.  Replace
 *   encode_delta_rowmajor_{8b,16b} / decode_delta_rowmajor_{8b,16b}              cpp/Compress/delta.h:17-24,53-60
 *   encode_doubledelta_rowmajor_{8b,16b} / decode_doubledelta_rowmajor_{8b,16b}  cpp/Compress/delta.h:36-43,63-68
 *   encode_xff_rowmajor_{8b,16b} / decode_xff_rowmajor_{8b,16b}                  cpp/Compress/predict.h:15-30
 * Per column (element index mod ndims), state starting at zero, arithmetic
 * wrapping at the element width: delta y[r] = x[r] - x[r-1]; double delta
 * y[r] = x[r] - 2 x[r-1] + x[r-2].  One call transforms ONE stream of any
 * length; the decode is a scan over its rows (transforms.hip): one pass -- a chained scan
 * over 128 KB tiles on persistent workgroups -- for 16-bit streams whose
 * rows are 1 .. 8 whole 16-byte pieces (or 2 / 4 / 8 bytes), two passes otherwise (env
 * SPRINTZ_MI355X_TRANSFORM_CHAIN: 0 = two passes always, n = one pass from n tiles on;
 * A/B runs, tests).  What d_tmp holds on entry does not matter (the one-pass form zeroes
 * the words it polls itself, hipMemsetAsync on the stream; every other array is written
 * before it is read), and it may be reused by the next call on the stream as it is.
 * SPRINTZ_TRANSFORM_XFF is the FIRE forecaster with no packing (errors out), with
 * predict.cpp's own constants (not the codec's); only whole 8-row blocks that its
 * vector stores cannot spill past the end are forecast, the rest is plain delta
 * (predict.cpp:96-103, :266-273).  Its counters make the rows of one stream strictly
 * sequential in both directions: a lane per column, latency-bound (transforms.hip).
 *   kind        : SPRINTZ_TRANSFORM_DELTA / SPRINTZ_TRANSFORM_DOUBLEDELTA / SPRINTZ_TRANSFORM_XFF
 * Device forms: len elements in, len elements out, no header;
 *   d_tmp: sprintz_mi355x_transform_tmp_bytes(kind, elem_bytes, len, ndims) bytes, 16-byte
 *   aligned: the most that any form of the decode takes for this shape, whatever the
 *   alignment of d_src and d_dest and whatever SPRINTZ_MI355X_TRANSFORM_CHAIN says -- it is
 *   derived from the launcher's own layout (csrc/transform_plan.h), so a caller can size
 *   the scratch before it knows either.
 * Host forms: the reference's container -- a 6-byte header {u32 len; u16 ndims}
 * (format.h:65-86) before the transformed elements; encode returns len + header
 * length in elements (6 @8b, 3 @16b; delta.cpp:120), decode returns len.  decode
 * with raw_len == raw_ndims == 0 reads the header; otherwise src is headerless
 * (the reference's 4-argument form, delta.h:19).
 * ---------------------------------------------------------------------- */
#define SPRINTZ_TRANSFORM_DELTA 0
#define SPRINTZ_TRANSFORM_DOUBLEDELTA 1
#define SPRINTZ_TRANSFORM_XFF 2
size_t sprintz_mi355x_transform_tmp_bytes(int kind, int elem_bytes, uint64_t len, uint16_t ndims);
int sprintz_mi355x_transform_encode_device(int kind, int elem_bytes, const void* d_src, uint64_t len, uint16_t ndims, void* d_dest,
                                           void* hip_stream);
int sprintz_mi355x_transform_decode_device(int kind, int elem_bytes, const void* d_src, uint64_t len, uint16_t ndims, void* d_dest,
                                           void* d_tmp, void* hip_stream);
int64_t sprintz_mi355x_transform_encode(int kind, int elem_bytes, const void* src, uint32_t len, void* dest, uint16_t ndims,
                                        int write_size);
int64_t sprintz_mi355x_transform_decode(int kind, int elem_bytes, const void* src, void* dest, uint32_t raw_len, uint16_t raw_ndims);
const char* sprintz_mi355x_transform_last_error(void);

/* ------------------------------------------------------------------------
 * The reference's 2020 "online" coders for 1-D uint16 streams.  Replace
 *   dynamic_delta_pack_u16 / dynamic_delta_pack_u16_altloss / dynamic_delta_unpack_u16   cpp/Compress/online.hpp:412-424
 *   zigzag_pack_u16 / zigzag_unpack_u16                                                  cpp/Compress/online.hpp:431-438
 *   sprintzpack_pack_u16 / _zigzag / sprintzpack_unpack_u16 / _zigzag                    cpp/Compress/online.hpp:450-462
 * One call codes ONE stream; the containers ({u32 len} + payload, restated in oracle/online_oracle.c) are byte-exact
 * with the reference on every byte it writes (it leaves header padding unwritten; here those bytes are 0).
 * Return values are ELEMENTS like the reference's.  Device forms: d_src / d_dest 16-byte aligned,
 * d_dest of sprintz_mi355x_online_bound() bytes, d_tmp of sprintz_mi355x_online_tmp_bytes(); *d_ret (device) receives the
 * return value -- for unpack, SPRINTZ_E_CORRUPT if the container's length field differs from `len`.
 * The dynamic-delta decoder takes streams of at least 128 tiles (of 8 192 blocks: 16 MB) in one pass -- a chained scan of the blocks' affine
 * maps on persistent workgroups -- and shorter ones in three launches (env SPRINTZ_MI355X_ONLINE_CHAIN: 0 = three launches always,
 * n = one pass from n tiles on; A/B runs, tests).
 * ---------------------------------------------------------------------- */
#define SPRINTZ_ONLINE_DYNDELTA 0        /* dynamic delta / double delta, loss SumLogAbs */
#define SPRINTZ_ONLINE_DYNDELTA_ALT 1    /* ... loss MaxAbs (encoder only differs) */
#define SPRINTZ_ONLINE_ZIGZAG 2
#define SPRINTZ_ONLINE_PACK 3            /* sprintzpack: per-block width + bit-packing, no zigzag */
#define SPRINTZ_ONLINE_PACK_ZIGZAG 4
size_t sprintz_mi355x_online_bound(int kind, uint32_t len);
size_t sprintz_mi355x_online_tmp_bytes(int kind, uint32_t len);
int sprintz_mi355x_online_pack_device(int kind, const uint16_t* d_src, uint32_t len, void* d_dest, int64_t* d_ret, void* d_tmp, void* hip_stream);
int sprintz_mi355x_online_unpack_device(int kind, const void* d_src, uint32_t len, uint16_t* d_dest, int64_t* d_ret, void* d_tmp, void* hip_stream);
int64_t sprintz_mi355x_online_pack(int kind, const uint16_t* src, uint32_t len, int16_t* dest);     /* host buffers */
int64_t sprintz_mi355x_online_unpack(int kind, const int16_t* src, uint16_t* dest);                 /* host buffers; len from the header */

/* ------------------------------------------------------------------------
 * Multi-GPU: one process per GPU, rank r owns a contiguous chunk range, the data
 * path has NO collective.  The only exchange is one all-gather of 8 bytes per rank -- each rank's
 * compressed byte count -- from which every rank derives where its container starts in the
 * job-wide one.  It runs over RCCL (xGMI), in-stream behind sprintz_mi355x_compact:
 *   rank 0:      sprintz_mi355x_comm_unique_id(id)   -> ship the 128 bytes to the other ranks
 *                                                        (any bootstrap: torchrun's store, MPI, a file)
 *   every rank:  sprintz_mi355x_comm_init(id, rank, world, &comm)          (on its own HIP device)
 *   per batch:   sprintz_mi355x_compact(..., d_offsets, ...)               d_offsets[nchunks] = local bytes
 *                sprintz_mi355x_gather_layout(comm, &d_offsets[nchunks], d_all, stream)   ncclAllGather
 *                sprintz_mi355x_layout_bases(d_all, world, bases, stream)  host: bases[r] = global byte offset
 *                                                                           of rank r's container, bases[world] = total
 * RCCL is loaded at run time (dlopen by SONAME; inside a torch process that is the copy
 * torch.distributed's "nccl" backend uses); without it comm_* return SPRINTZ_E_UNSUPPORTED.
 * ---------------------------------------------------------------------- */
#define SPRINTZ_MI355X_COMM_ID_BYTES 128
int sprintz_mi355x_comm_unique_id(void* id_out);
int sprintz_mi355x_comm_init(const void* id, int rank, int world, void** comm_out);
int sprintz_mi355x_gather_layout(void* comm, const uint64_t* d_local_total, uint64_t* d_all, void* hip_stream);
int sprintz_mi355x_layout_bases(const uint64_t* d_all, int world, uint64_t* bases_out /* world + 1 */, void* hip_stream);
int sprintz_mi355x_comm_destroy(void* comm);

/* ------------------------------------------------------------------------
 * Host convenience: chunked codec over host buffers (what lzbench does per
 * block).  Stages through device memory; PCIe-inclusive by construction.
 * comp layout: chunk streams concatenated byte-dense; offsets[nchunks+1].
 * ---------------------------------------------------------------------- */
int64_t sprintz_mi355x_compress_chunked_host(int codec, int elem_bytes, const void* src, uint64_t total_len,
                                             uint32_t chunk_len, uint16_t ndims,
                                             void* comp, size_t comp_capacity, uint64_t* offsets);
int64_t sprintz_mi355x_decompress_chunked_host(int codec, int elem_bytes, const void* comp,
                                               const uint64_t* offsets, uint64_t nchunks,
                                               uint32_t chunk_len, uint16_t ndims, void* out);

#ifdef __cplusplus
}
#endif
#endif /* SPRINTZ_MI355X_H */
