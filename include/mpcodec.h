/*
 * mpcodec.h -- C ABI of libmpcodec.so: the MI355X (gfx950) drop-in for the
 * CompressionLib per-tile encode path of mnesbit/ImageExperiments.
 *
 * Plain pointers and sizes only; no exceptions cross this boundary (the
 * reference throws heap-allocated std::range_error*; here every entry point
 * returns an mpc_status and mpc_last_error() carries the text).
 * Citations are relative to the reference tree (/root/reference).
 *
 * Reference interface each entry point replaces:
 *   mpc_context_create        compressed::createCompressionContext        CompressionLib/inc/CompressedImage.h:54
 *                             (createQuantizationTables CompressedImage.cpp:124, distinctLineShapes BasisSet.cpp:204,
 *                              createSegmentDictionary :299, createIntraSegmentDictionary :513)
 *   mpc_context_get/set_quant CompressionContext::{Y,U,V}.Quant           CompressedImage.h:22-36 (Compression.cpp:104-110
 *                                                                          overwrites them for "max" quality)
 *   mpc_encode_batch_device   (same, several frames per launch)
 *   mpc_encode_tiles_device   the tile loop of compressed::encodeImage    CompressedImage.cpp:535-573, i.e. per tile
 *   mpc_encode_tiles          and channel: gather + img::YUVFromRGB (misc.cpp:7) + matching::CalcMPDynamic
 *                             (MatchingPursuit.h:22, MatchingPursuit.cpp:39) over compressed::dynamicBasis
 *                             (CompressedImage.cpp:212)
 *   mpc_histogram_device      (new) per-stream symbol counts feeding huffman::huffmanEncode / golombCodeLength
 *                             (CompressedImage.cpp:359-379); the multi-GPU all-reduce operand
 *   mpc_calc_mp               matching::CalcMPDynamic on one vector       MatchingPursuit.h:22 (Compression.cpp:250 "-s" mode)
 *   mpc_write_compressed      compressed::writeCompressed (static)        CompressedImage.cpp:403
 *   mpc_read_compressed       compressed::readCompressed                  CompressedImage.cpp:635
 *   mpc_encode_image          compressed::encodeImage                     CompressedImage.h:59
 *   mpc_encode_images         (same, a sequence of frames, host and device stages overlapped)
 *   mpc_encode_image(s)_device (same, frames already in device memory)
 *   mpc_encode_images_indexed[_device] (same, each container together with its seek index: the blob mpc_container_index
 *                             would build from it, emitted by the entropy stage instead of parsed out of the finished bytes;
 *                             mpc_code_symbol_streams_device_indexed, mpc_assemble_symbol_streams_by_plan_indexed: the
 *                             entropy stage alone, on the device and on the host)
 *   mpc_encode_images_indexed2[_device] (same with `flags`: MPC_INDEX_EXPANDED = index version 2, the aux entries from the
 *                             entropy stage's run-length pack kernel as well; mpc_code_symbol_streams_device_indexed2,
 *                             mpc_assemble_symbol_streams_by_plan_indexed2)
 *   mpc_decode_image          compressed::decodeImage                     CompressedImage.h:75
 *   mpc_decode_tiles_device   matching::FromCoeffsDynamic per tile        MatchingPursuit.h:25, CompressedImage.cpp:797-831
 *   mpc_psnr                  compressed::calculatePSNR                   CompressedImage.h:57
 *   mpc_quant_tables          compressed::createQuantizationTables        CompressedImage.cpp:124-166 (without a context)
 *   mpc_distortion_device     (new) calculatePSNR's sum of squares of decodeImage's reconstruction, from the records
 *   mpc_rate_distortion       Compression.cpp -n / -g for one frame        Compression.cpp:144-182, :303-350
 *   mpc_rate_distortion_device (same, frame already in device memory)
 *   mpc_huffman_encode/decode huffman::huffmanEncode / huffmanDecode      Huffman.h:15-19
 *   mpc_rle_encode/decode     huffman::runLengthEncode / runLengthDecode  Huffman.h:12-13
 */
#ifndef MPCODEC_H
#define MPCODEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPC_MAX_K 32
#define MPC_HIST_BINS 8192

typedef enum {
    MPC_OK = 0,
    MPC_ERR_ARGUMENT = 1,      /* bad K / block size / null pointer / geometry            */
    MPC_ERR_NO_DEVICE = 2,     /* context has no GPU (created with device < 0) or HIP failed to initialise */
    MPC_ERR_HIP = 3,           /* a HIP runtime call failed; see mpc_last_error            */
    MPC_ERR_BITSTREAM = 4,     /* "Invalid input data" / "Invalid bitstream" of the reference */
    MPC_ERR_ALLOC = 5
} mpc_status;

/* matching::BasisChoice, MatchingPursuit.h:13-17 (same layout: two u16) */
typedef struct {
    uint16_t deltaId;
    uint16_t intCoeff;
} mpc_basis_choice;

typedef struct mpc_context mpc_context;

const char* mpc_version(void);
/* text of the last failure on this thread (never NULL) */
const char* mpc_last_error(void);

/* K in 1..32, block_size must be 8 for the device path (host-only contexts accept 1..8).
 * device >= 0: HIP device ordinal, dictionary uploaded once; device < 0: host-only context
 * (dictionary/quant queries and the bitstream entry points work, encode_tiles does not). */
mpc_status mpc_context_create(int K, int block_size, double bpp_allocation, int device, mpc_context** out);
void mpc_context_destroy(mpc_context* ctx);

int mpc_context_K(const mpc_context* ctx);
int mpc_context_block_size(const mpc_context* ctx);
int mpc_context_num_base(const mpc_context* ctx);          /* 510 for 8x8 */
int mpc_context_detail_rows(const mpc_context* ctx);       /* 31622 for 8x8, per channel */
int mpc_context_device(const mpc_context* ctx);
int mpc_context_max_waves(const mpc_context* ctx);          /* resident waves of the encode kernel on the device */

/* The `...Fast` flavour of the tile path (CompressionLib/inc/MatchingPursuit.h:23,26, CompressedImage.h:67-76 -- what
 * Compression.cpp itself calls): residual, projections, quantisation, update and reconstruction in float on the dictionary
 * rounded to float.  on != 0 switches every encode / decode entry point of this context to it; the container format and the
 * entropy stage are the double path's.  PARITY UNPINNED: the reference's float results come from Eigen (absent from the
 * tree) on a dictionary built by Eigen's float eigensolver; what runs here is the reference's statements read literally in
 * float (sequential sums, products and sums rounded separately), bit-identical to oracle/mpo_fast.c and equivalent to the
 * double path in PSNR and size, not in bytes. */
mpc_status mpc_context_set_fast(mpc_context* ctx, int on);

/* How many CUs the tile encode (mpc_encode_tiles[_device], mpc_encode_batch_device) may fill: `workgroups` persistent
 * workgroups, one per CU; 0 = all of them (the default).  For callers that keep other work on the device beside it -- a
 * stripe exchange and the container jobs of the previous step (imageexperiments_amd/sharding.py: StripedEncoder.run) -- what
 * mpc_encode_images[_device] does by itself for a frame sequence: leave one CU in eight, one per shader engine, free
 * (mpc_context_max_waves / 12 = the CUs).  Not a reference interface: the reference has no device. */
mpc_status mpc_context_set_tile_encode_workgroups(mpc_context* ctx, int workgroups);
int mpc_context_is_fast(const mpc_context* ctx);

/* quant[3*K]: Y then U then V */
mpc_status mpc_context_get_quant(const mpc_context* ctx, double* quant);
mpc_status mpc_context_set_quant(mpc_context* ctx, const double* quant);

/* Copies of the host dictionary (any pointer may be NULL):
 * base[num_base*64], block_rows[num_base], detail_{y,u,v}[detail_rows*64] */
mpc_status mpc_context_get_dictionary(const mpc_context* ctx, double* base, int32_t* block_rows,
                                      double* detail_y, double* detail_u, double* detail_v);

/* ---- the hot path -------------------------------------------------------------------------------------
 * Encodes the tile rows [tile_row_begin, tile_row_end) of one RGB frame resident in device memory.
 * d_rgb: row-major, 3 bytes per pixel, `row_stride` bytes between rows (img::image<rgb>, image.h:123-131).
 * Tiles outside the image are zero filled (CompressedImage.cpp:548-552).
 * The frame's layout (this entry point, the batch form and the host form alike): pixel (x, y) is the 3 bytes at
 * d_rgb + y * row_stride + 3 * x, row_stride >= 3 * width, so the frame may be a window of a larger image.  Only pixel
 * bytes are read: the last row needs 3 * width bytes, not a full stride, and the bytes between the end of a row and the
 * next row (and between the frames of a batch) are never read, whatever they hold.  Any alignment of d_rgb, row_stride
 * and frame_stride is accepted; a base and strides that are multiples of 8 bytes take a faster pixel fetch.
 * MPC_ERR_ARGUMENT, with nothing read, enqueued or written: a null pointer, width or height < 1, row_stride < 3 * width,
 * tile rows not within 0 <= tile_row_begin < tile_row_end <= ceil(height / 8).
 * Outputs (device memory, caller allocated), tile index t = tx * rows + (ty - tile_row_begin), rows =
 * tile_row_end - tile_row_begin, i.e. the reference's x-outer / y-inner order within the stripe:
 *   d_counts [tiles][3]      u16   CalcMPDynamic's return value per channel (Y,U,V)
 *   d_choices[tiles][3][K]         records 0..count (the terminating record is written as the reference
 *                                   writes it, MatchingPursuit.cpp:50-69); entries beyond are zero
 *   d_energy [tiles][3]      f64   sum of squares of the final residual (diagnostic, not in CompressionLib)
 *   d_swept  [tiles][3]      u32   dictionary rows correlated, SURVEY 8(d) "S"
 * d_energy / d_swept may be NULL.  quant: host pointer to 3*K doubles or NULL for the context's tables.
 * stream: hipStream_t (NULL = default stream).  Asynchronous; no synchronisation, and no allocation once the
 * workspace covers the call (mpc_reserve): that holds with a quant override too, which is read before the call returns.
 * waves: reserved, pass 0.
 * Streams and graphs, for this and every other entry point with a `stream` argument (the mpc_debug_* probes included): the work is ordered on `stream` like a
 * kernel launch of the caller's own (behind what `stream` holds, in front of what is enqueued next), whatever other streams
 * other calls of the context or the process use.  A stream that is being captured into a graph (hipStreamBeginCapture) is
 * refused with MPC_ERR_ARGUMENT before anything is enqueued, and the capture stays valid: the calls of a process share scratch
 * in an order that a replayed graph would take no part in. */
mpc_status mpc_encode_tiles_device(mpc_context* ctx, const uint8_t* d_rgb, int width, int height, size_t row_stride,
                                   int tile_row_begin, int tile_row_end, const double* quant,
                                   uint16_t* d_counts, mpc_basis_choice* d_choices, double* d_energy, uint32_t* d_swept,
                                   int waves, void* stream);

/* Batch form: `frames` equally sized frames, `frame_stride` bytes apart; the same tile rows of every frame are
 * encoded in ONE launch (BASELINE config 4: batches of frames row-striped across GPUs).
 * Output tile index t = frame * tiles_per_stripe + tx * rows + (ty - tile_row_begin).
 * Frame f starts at d_rgb + f * frame_stride; frames = 1 ignores frame_stride.  MPC_ERR_ARGUMENT also for frames < 1 and,
 * with frames > 1, for frame_stride < row_stride * height. */
mpc_status mpc_encode_batch_device(mpc_context* ctx, const uint8_t* d_rgb, int frames, size_t frame_stride,
                                   int width, int height, size_t row_stride, int tile_row_begin, int tile_row_end,
                                   const double* quant, uint16_t* d_counts, mpc_basis_choice* d_choices,
                                   double* d_energy, uint32_t* d_swept, int waves, void* stream);

/* Same with host buffers: uploads the frame, runs the kernel, copies the records back, synchronises.  The arguments are
 * checked before rgb is read; then exactly (height - 1) * row_stride + 3 * width bytes are read from it. */
mpc_status mpc_encode_tiles(mpc_context* ctx, const uint8_t* rgb, int width, int height, size_t row_stride,
                            int tile_row_begin, int tile_row_end, const double* quant,
                            uint16_t* counts, mpc_basis_choice* choices, double* energy, uint32_t* swept);

/* d_hist[(1 + 6K)][MPC_HIST_BINS] u32 += symbol counts of the records of `tiles` tiles:
 * row 0 = lengths, row 1 + 2K*ch + 2i = deltaId at step i, +1 = intCoeff at step i. Asynchronous. */
mpc_status mpc_histogram_device(mpc_context* ctx, const uint16_t* d_counts, const mpc_basis_choice* d_choices,
                                long long tiles, uint32_t* d_hist, void* stream);

/* matching::CalcMPDynamic on one 64-vector on the device (Compression.cpp -s mode); channel 0/1/2.
 * choices[K]; *count receives the return value. Synchronous. */
mpc_status mpc_calc_mp(mpc_context* ctx, int channel, const double* quant_k, const double* input64,
                       mpc_basis_choice* choices, int* count);

/* Batch form: `count` vectors inputs[count][64] of one channel; counts[count], choices[count][K];
 * energy[count] / swept[count] optional. quant_k: K steps for that channel or NULL = context table. */
mpc_status mpc_calc_mp_batch(mpc_context* ctx, int channel, const double* quant_k, const double* inputs, int count,
                             mpc_basis_choice* choices, uint16_t* counts, double* energy, uint32_t* swept);

/* Pre-allocates the device workspace for calls of up to max_tiles tiles (3 tile-channels each).  The encode
 * entry points grow the workspace on demand, which synchronises the device; callers that must not synchronise
 * reserve first.  A call is cut into sub-batches that run on two internal streams (forked from and
 * joined to the caller's stream with events); at most 262144 tiles are in flight. */
mpc_status mpc_reserve(mpc_context* ctx, long long max_tiles);

/* Live timing of the dominant kernel (mp_pursuit_kernel, one launch per channel): while enabled every launch of it is
 * bracketed by HIP events on the stream it is launched on.  mpc_kernel_timing_read synchronises and returns, for
 * the launches since the last read/enable: the summed duration, their number, and (busy_ms, may be NULL) the
 * length of the union of their intervals -- launches of the two internal streams overlap.  Measurement only. */
void mpc_kernel_timing_enable(mpc_context* ctx, int on);
/* What the pursuit kernel itself counted since mpc_kernel_timing_enable(ctx, 1) or the last read (every wave adds its tallies
 * once, at exit): v_mfma_f32_16x16x32_bf16 instructions executed (16384 flop each) and tile-channel-steps.  Synchronises. */
mpc_status mpc_kernel_counters_read(mpc_context* ctx, unsigned long long* mfma_instructions, unsigned long long* tile_channel_steps);
mpc_status mpc_kernel_timing_read(mpc_context* ctx, double* total_ms, long long* launches, double* busy_ms);

/* ---- host entropy stage and container (stays on the host; bytes identical to the reference) ----------
 * Buffers returned through `uint8_t**` / `uint16_t**` are malloc'ed by the library: release with mpc_free. */
typedef struct mpc_streams mpc_streams;

void mpc_free(void* p);

/* writeCompressed (CompressedImage.cpp:403): header, DC differencing of codes[1], [2K+1], [4K+1], optional RLE,
 * Huffman-or-Golomb per stream.  quant[3*K]; lengths = 3 per tile in x-outer / y-inner tile order;
 * codes[6K] / code_lengths[6K] = the streams codes[2K*ch + 2i] (deltaId) and [+1] (intCoeff) as the encoder
 * holds them (DC coefficients NOT yet differenced). */
mpc_status mpc_write_compressed(int width, int height, int K, int block_size, const double* quant,
                                const uint16_t* lengths, size_t n_lengths, const uint16_t* const* codes,
                                const size_t* code_lengths, uint8_t** bytes, size_t* nbytes);

/* The host half of encodeImage (CompressedImage.cpp:555-575): per-tile records of a WHOLE frame, tile
 * t = tx*tiles_y + ty (what mpc_encode_tiles returns for rows [0, tiles_y)), -> container bytes. */
mpc_status mpc_assemble_streams(int width, int height, int K, int block_size, const double* quant,
                                const uint16_t* counts, const mpc_basis_choice* choices, uint8_t** bytes, size_t* nbytes);

/* Same container from records in planar order, planar[(channel * K + step) * tiles + t]: each stream's records are
 * then one contiguous run for the host.  (mpc_encode_image assembles its streams on the device and uses neither.) */
mpc_status mpc_assemble_planar_streams(int width, int height, int K, int block_size, const double* quant,
                                       const uint16_t* counts, const mpc_basis_choice* planar, uint8_t** bytes, size_t* nbytes);

/* Same container from streams that are already assembled (what the device's stream assembly hands the host): symbols =
 * codes[0] ++ codes[1] ++ ... ++ codes[6K-1], live symbols only, tiles in the reference's order, the three step-0 coefficient
 * streams ALREADY difference coded (CompressedImage.cpp:428-446); stream_off[6K + 1] = their boundaries in `symbols`. */
mpc_status mpc_assemble_symbol_streams(int width, int height, int K, int block_size, const double* quant, const uint16_t* counts,
                                       const uint16_t* symbols, const unsigned long long* stream_off, uint8_t** bytes, size_t* nbytes);

/* The same container by the route the device-side entropy stage takes (per-stream statistics -> Huffman table or Golomb M
 * and bit offsets -> codes written at their offsets), with the device's share computed on the host: a host-only check of
 * the planning half against mpc_assemble_symbol_streams. */
mpc_status mpc_assemble_symbol_streams_by_plan(int width, int height, int K, int block_size, const double* quant, const uint16_t* counts,
                                               const uint16_t* symbols, const unsigned long long* stream_off, uint8_t** bytes, size_t* nbytes);

/* The entropy stage of writeCompressed (CompressedImage.cpp:403-460: run-length decision, Huffman-or-Golomb choice, coding)
 * for streams the caller holds in host memory, with the per-symbol work on the device (mp_entropy.hip): run lengths,
 * histograms and first appearances are taken on the device, the host builds one code table per stream, the device writes
 * the codes.  Inputs as for mpc_assemble_symbol_streams (counts[3 * tiles] is the `lengths` stream; K and block size are the
 * context's; quant NULL = the context's tables); same bytes.  *route (optional): 0 = coded on the device, 1 = a stream was
 * outside what the device tables hold (or MPC_HOST_ENTROPY=1) and the host coded the container. */
mpc_status mpc_code_symbol_streams_device(mpc_context* ctx, int width, int height, const double* quant, const uint16_t* counts,
                                          const uint16_t* symbols, const unsigned long long* stream_off, uint8_t** bytes, size_t* nbytes,
                                          int* route);

/* The two above with the container's seek index (mpc_encode_images_indexed): *index / *index_bytes receive what
 * mpc_container_index(*bytes, *nbytes, interval, ...) would return.  The by-plan form records the checkpoints while it writes the
 * codes on the host and so defines, without a GPU, what the device's code kernel records.  Both accept streams that do not hold
 * what `counts` implies (every stream as many symbols as tiles of its channel have more atoms than its step; only a test makes
 * other streams): no parser accepts that container, so it comes back alone, *index = NULL, *index_bytes = 0, MPC_OK. */
mpc_status mpc_assemble_symbol_streams_by_plan_indexed(int width, int height, int K, int block_size, const double* quant,
                                                       const uint16_t* counts, const uint16_t* symbols, const unsigned long long* stream_off,
                                                       int interval, uint8_t** bytes, size_t* nbytes, uint8_t** index, size_t* index_bytes);
mpc_status mpc_code_symbol_streams_device_indexed(mpc_context* ctx, int width, int height, const double* quant, const uint16_t* counts,
                                                  const uint16_t* symbols, const unsigned long long* stream_off, int interval,
                                                  uint8_t** bytes, size_t* nbytes, uint8_t** index, size_t* index_bytes, int* route);

/* readCompressed (CompressedImage.cpp:635): parse a container; streams come back with the DC differencing
 * undone.  index -1 = lengths, 0..6K-1 = codes[index].  The expansion runs on the host.  The decoder expands on the device
 * and uses this only to name the status of a container it refuses for its block size or a length above K; it is the
 * reference for what the decoder accepts. */
mpc_status mpc_read_compressed(const uint8_t* bytes, size_t nbytes, mpc_streams** out);
mpc_status mpc_streams_info(const mpc_streams* s, int* width, int* height, int* K, int* block_size);
mpc_status mpc_streams_quant(const mpc_streams* s, uint16_t* quant /* [3*K] */);
size_t mpc_streams_length(const mpc_streams* s, int index);
mpc_status mpc_streams_copy(const mpc_streams* s, int index, uint16_t* dst);
void mpc_streams_free(mpc_streams* s);

/* The serial half of readCompressed on its own (host only; uses no worker pool and no shared state: containers may be parsed on
 * several threads side by side): an mpc_streams handle whose streams are the CODED ones, as entropy-decoded: still run-length
 * packed where the container's flag says so, the three step-0 coefficient streams (1, 2K + 1, 4K + 1) still difference coded.
 * mpc_streams_length / _copy / _info / _quant / _free work on it as on mpc_read_compressed's (index -1 = lengths, the same in
 * both). */
mpc_status mpc_read_compressed_coded(const uint8_t* bytes, size_t nbytes, mpc_streams** out);
/* 1 = stream `index` is run-length packed; 0 for every stream of a handle of mpc_read_compressed */
int mpc_streams_packed(const mpc_streams* s, int index);
/* symbols stream `index` must expand to (from the lengths stream) */
size_t mpc_streams_expected(const mpc_streams* s, int index);
/* The container's header alone (host only): lets a caller size device buffers.  MPC_ERR_BITSTREAM for a header
 * mpc_read_compressed refuses (too short, wrong magic, K, block size or geometry out of range). */
mpc_status mpc_container_info(const uint8_t* bytes, size_t nbytes, int* width, int* height, int* K, int* block_size);

/* huffman::huffmanEncode / huffmanDecode (Huffman.h:15-19), runLengthEncode / runLengthDecode (:12-13) */
mpc_status mpc_huffman_encode(const uint16_t* data, size_t n, uint8_t** bytes, size_t* nbytes);
mpc_status mpc_huffman_decode(const uint8_t* bytes, size_t nbytes, uint16_t** data, size_t* n);
mpc_status mpc_rle_encode(const uint16_t* data, size_t n, uint16_t** out, size_t* n_out);
mpc_status mpc_rle_decode(const uint16_t* data, size_t n, uint16_t** out, size_t* n_out);

/* Bit-level primitives of bitbuffer:: (CompressionLib/inc/BitBuffer.h) as the entropy stage uses them; the property tests of
 * Testing/BitBufferTests.cpp:37-247 run against these (tests/test_bit_primitives.py).
 *   mpc_bits_pack / _unpack      BitBuffer::WriteBits / ReadBits + Save / Load (MSB first, widths 0..64; reads past the end give 0)
 *   mpc_zigzag_*                 zigzagEncode / zigzagDecode                    BitBuffer.h:112-118
 *   mpc_golomb_*                 golombCodeLength / writeGolombCode / readGolombCode   BitBuffer.cpp:228-269
 *   mpc_elias_fano_*             eliasFanoSequenceCodeLength / write / read           BitBuffer.cpp:292-354 */
mpc_status mpc_bits_pack(const uint64_t* values, const int* widths, size_t n, uint8_t** bytes, size_t* nbytes, size_t* nbits);
mpc_status mpc_bits_unpack(const uint8_t* bytes, size_t nbytes, const int* widths, size_t n, uint64_t* values, size_t* remaining_bits);
uint32_t mpc_zigzag_encode(int32_t x);
int32_t mpc_zigzag_decode(uint32_t x);
uint32_t mpc_golomb_length(uint32_t value, uint32_t m);
mpc_status mpc_golomb_encode(const uint32_t* values, size_t n, uint32_t m, uint8_t** bytes, size_t* nbytes, size_t* nbits);
mpc_status mpc_golomb_decode(const uint8_t* bytes, size_t nbytes, size_t n, uint32_t m, uint32_t* values, size_t* remaining_bits);
uint32_t mpc_elias_fano_length(size_t n, uint16_t max_symbol);
mpc_status mpc_elias_fano_encode(const uint16_t* sorted, size_t n, uint16_t max_symbol, uint8_t** bytes, size_t* nbytes, size_t* nbits);
mpc_status mpc_elias_fano_decode(const uint8_t* bytes, size_t nbytes, size_t n, uint16_t max_symbol, uint16_t* sorted, size_t* remaining_bits);

/* compressed::encodeImage (CompressedImage.h:59): rgb host buffer, 3*width bytes per row; quant NULL = context
 * tables.  Tile encode, stream assembly and the per-symbol work of the entropy stage (run lengths, histograms, code writing)
 * on the device; the host builds one code table per stream; only the finished container crosses PCIe (a frame whose streams do
 * not fit the device tables takes the host route for the entropy stage: same bytes). */
mpc_status mpc_encode_image(mpc_context* ctx, const uint8_t* rgb, int width, int height, const double* quant,
                            uint8_t** bytes, size_t* nbytes);

/* The same for a sequence of equally sized frames (what Compression.cpp does per input file, :117/:166), pipelined: the
 * code tables of frame n are built on the host while the device encodes frame n+1.  bytes[i] / nbytes[i] receive frame i's
 * container (each to be released with mpc_free); byte-identical to n calls of mpc_encode_image.  On failure nothing is
 * returned. */
mpc_status mpc_encode_images(mpc_context* ctx, const uint8_t* const* rgb_frames, int n_frames, int width, int height,
                             const double* quant, uint8_t** bytes, size_t* nbytes);

/* The same two with the frames already resident in device memory (3*width bytes per row, tightly packed): what bench.py
 * times. */
mpc_status mpc_encode_image_device(mpc_context* ctx, const uint8_t* d_rgb, int width, int height, const double* quant,
                                   uint8_t** bytes, size_t* nbytes);
mpc_status mpc_encode_images_device(mpc_context* ctx, const uint8_t* const* d_rgb_frames, int n_frames, int width, int height,
                                    const double* quant, uint8_t** bytes, size_t* nbytes);

/* mpc_encode_images / mpc_encode_images_device with every frame's seek index (see "Seek index" below): indexes[i] /
 * index_bytes[i] receive the blob mpc_container_index(bytes[i], nbytes[i], interval, ...) would return, byte for byte, without
 * the container being parsed: the entropy stage knows where every stream begins and its code-writing kernel passes every
 * interval-th coded symbol's bit anyway.  The containers are those of the calls without an index.  interval as for
 * mpc_container_index (0 = the default; anything else outside 32 ... 65536 is MPC_ERR_ARGUMENT before anything is enqueued).
 * A frame that takes the host route for its entropy stage gets its index from the finished container on the host.
 * These return index version 1; mpc_encode_images_indexed2[_device] (below, "Index version 2") return version 2.
 * n_frames == 1 is the single-frame route (mpc_encode_image).  Every buffer is released with mpc_free; on failure nothing is
 * returned. */
mpc_status mpc_encode_images_indexed(mpc_context* ctx, const uint8_t* const* rgb_frames, int n_frames, int width, int height,
                                     const double* quant, int interval, uint8_t** bytes, size_t* nbytes, uint8_t** indexes,
                                     size_t* index_bytes);
mpc_status mpc_encode_images_indexed_device(mpc_context* ctx, const uint8_t* const* d_rgb_frames, int n_frames, int width, int height,
                                            const double* quant, int interval, uint8_t** bytes, size_t* nbytes, uint8_t** indexes,
                                            size_t* index_bytes);

/* compressed::encodeImage for a sequence of equally sized frames on SEVERAL GPUs of one node from one process (what a
 * Compression.cpp-style caller gets with MPC_DEVICES=0,1,...: dropin/compressionlib_dropin.cpp).  ctxs[0 .. n_devices): one context
 * per lane, each created on the device the lane shall use (two lanes may name the same device, not the same context), same K and
 * the same flavour (mpc_context_set_fast), and with quant == NULL the same quantiser tables: a frame's stripes meet in one
 * container, so lanes that differ in any of these are refused with MPC_ERR_ARGUMENT (an explicit `quant` makes different context
 * tables harmless and is allowed).
 * Every frame's tile rows are striped over the lanes (contiguous stripes, remainder to the first lanes); a step takes
 * n_devices frames, frame f of a step is owned by lane f, which pulls the other lanes' stripes of it (hipMemcpyPeerAsync), puts
 * them into the reference's tile order and produces the container.  bytes[i] / nbytes[i]: frame i's container (mpc_free),
 * byte-identical to mpc_encode_image.  n_devices == 1 is mpc_encode_images. */
mpc_status mpc_encode_images_multi(mpc_context* const* ctxs, int n_devices, const uint8_t* const* rgb_frames, int n_frames,
                                   int width, int height, const double* quant, uint8_t** bytes, size_t* nbytes);

/* Multi-GPU path, between the stripe exchange and the stream assembly: the records of tile rows [tile_row_begin, tile_row_end)
 * of a frame, in the order mpc_encode_tiles_device writes a stripe (t = tx*rows + ty_local), copied to their places in the whole
 * frame's records (t = tx*tiles_y + ty: the reference's visiting order, CompressedImage.cpp:535-537).  Asynchronous on `stream`. */
mpc_status mpc_interleave_stripe_device(mpc_context* ctx, const uint16_t* d_part_counts, const mpc_basis_choice* d_part_choices,
                                        int width, int height, int tile_row_begin, int tile_row_end, uint16_t* d_frame_counts,
                                        mpc_basis_choice* d_frame_choices, void* stream);

/* The second half of encodeImage (CompressedImage.cpp:555-575) for records that are already in device memory in whole-frame
 * order, tile t = tx*tiles_y + ty (a frame's owner in the multi-GPU path after the stripe exchange): stream assembly on the
 * device (on `stream`), live symbols to the host, entropy stage.  Synchronises `stream`. */
mpc_status mpc_records_to_container_device(mpc_context* ctx, const uint16_t* d_counts, const mpc_basis_choice* d_choices, int width,
                                           int height, const double* quant, void* stream, uint8_t** bytes, size_t* nbytes);
/* The same in three steps, for a caller that keeps the device busy meanwhile (the multi-GPU path: the next step's tile encode
 * runs while this frame's code tables are built).  slot in [0, MPC_JOB_SLOTS): one job per slot at a time; the records must
 * stay untouched until `collect` has returned (the counts are the `lengths` stream the last kernels read).
 *   begin    stream assembly and the first phase of the entropy stage enqueued on `stream`; nothing is waited for
 *   tables   waits for that, builds the code tables on the host, enqueues the second phase and the container's copy on `stream`
 *   collect  waits for the copy; the container (mpc_free)
 * A job owns its buffers: any other entry point of the context (mpc_encode_image(s), mpc_decode_image, ...) may be called between
 * `begin` and `collect`; calls on one context are serialised, not forbidden. */
#define MPC_JOB_SLOTS 6
mpc_status mpc_container_job_begin(mpc_context* ctx, int slot, const uint16_t* d_counts, const mpc_basis_choice* d_choices, int width,
                                   int height, const double* quant, void* stream);
mpc_status mpc_container_job_tables(mpc_context* ctx, int slot);
mpc_status mpc_container_job_collect(mpc_context* ctx, int slot, uint8_t** bytes, size_t* nbytes);
/* Gives a slot up whatever step its job is at (a caller that failed elsewhere between `begin` and `collect`): waits for what the
 * job has enqueued, drops its result, leaves the slot idle.  An idle slot: no-op. */
mpc_status mpc_container_job_cancel(mpc_context* ctx, int slot);

/* matching::FromCoeffsDynamic (MatchingPursuit.h:25) + img::RGBFromYUV for every tile of a frame on the device:
 * records in the reference's order (tile t = tx*tiles_y + ty, as mpc_encode_tiles returns them for the whole
 * frame), d_rgb = height*width*3 bytes.  quant: host [3*K] or NULL = context tables.  Asynchronous. */
mpc_status mpc_decode_tiles_device(mpc_context* ctx, const uint16_t* d_counts, const mpc_basis_choice* d_choices,
                                   const double* quant, int width, int height, uint8_t* d_rgb, void* stream);

/* compressed::decodeImage (CompressedImage.h:75): mpc_decode_images below, entered with one frame (the same code; the parse
 * runs on the calling thread).  The entropy codes are parsed on the host, everything behind them happens on ctx's device, with
 * the K and quantisation tables the stream carries (they need not equal the context's; the block size must).  Returns when
 * this frame's pixels are complete; it waits for no other work on the device.  On failure *rgb holds no buffer and
 * mpc_last_error says what was wrong (no frame index in front).  A context without a device gets MPC_ERR_NO_DEVICE: there
 * is no host reconstruction. */
mpc_status mpc_decode_image(const mpc_context* ctx, const uint8_t* bytes, size_t nbytes, uint8_t** rgb, int* width,
                            int* height);

/* compressed::decodeImage for n containers in one call (sizes, K and tables may differ from frame to frame; the block size must
 * be the context's): the containers are parsed side by side on threads of the call's own (only what the format makes serial: the
 * entropy codes), the coded streams cross PCIe, run lengths and DC differences are undone on the device (mp_unpack.hip) in
 * front of the gather and the reconstruction, frames pipelined over slots.  rgb[i] (mpc_free) / width[i] / height[i] per frame;
 * one implementation serves every n, so a frame's pixels do not depend on the call it was decoded in.  n_frames < 1 is
 * MPC_ERR_ARGUMENT.  On failure nothing is returned; mpc_last_error names the first failing frame ("frame N: ..."), the status is
 * that container's: MPC_ERR_BITSTREAM for whatever mpc_read_compressed refuses and for a record outside its dictionary,
 * MPC_ERR_ARGUMENT for a block size that is not the context's. */
mpc_status mpc_decode_images(mpc_context* ctx, const uint8_t* const* bytes, const size_t* nbytes, int n_frames, uint8_t** rgb,
                             int* width, int* height);
/* The same with the pixels left in device memory: d_rgb[i] is caller-allocated on ctx's device, capacity[i] bytes >= 3*w*h of
 * frame i (else MPC_ERR_ARGUMENT before anything is enqueued; mpc_container_info gives w and h), rows tightly packed; bytes
 * behind 3*w*h are not touched.  Returns when every frame's pixels are complete. */
mpc_status mpc_decode_images_device(mpc_context* ctx, const uint8_t* const* bytes, const size_t* nbytes, int n_frames,
                                    uint8_t* const* d_rgb, const size_t* capacity, int* width, int* height);
mpc_status mpc_decode_image_device(mpc_context* ctx, const uint8_t* bytes, size_t nbytes, uint8_t* d_rgb, size_t capacity,
                                   int* width, int* height);
/* The device half of that on its own, for tests (the counterpart of mpc_code_symbol_streams_device): host buffers in and out.
 * coded = the 6K streams as entropy-decoded, back to back, stream i at [coded_off[i], coded_off[i + 1]); is_packed[6K];
 * expect[6K].  symbols (mpc_free): sum(expect) u16, the streams expanded and the DC streams summed, back to back.  A stream
 * that does not expand to exactly expect[i] symbols: MPC_ERR_BITSTREAM. */
mpc_status mpc_unpack_symbol_streams_device(mpc_context* ctx, int K, const uint16_t* coded, const unsigned long long* coded_off,
                                            const uint8_t* is_packed, const unsigned long long* expect, uint16_t** symbols,
                                            size_t* n_symbols);

/* ---- seek index: the entropy codes parsed on the device ("Seek index") ----
 * The container format is serial for one reason: a stream's first bit is known once the stream before it has been decoded, and
 * a code's first bit once the code before it has.  An index holds where every one of the 1 + 6K streams begins and where every
 * interval-th coded symbol of it begins; with it every chunk of `interval` symbols decodes on its own.  The container's bytes
 * stay the reference's; the index is a separate blob a caller keeps beside a container it will decode more than once.
 * An index is a hint, never an authority: a decode with one gives the pixels, status and error text of a decode without one,
 * whatever the index holds (a damaged one, another container's).  Its structure is checked against the container on the host,
 * every chunk must yield exactly its symbols and end exactly where the next begins (on the pseudo-EOF and the stream's end for
 * the last), and the expected stream sizes are recomputed from the decoded lengths; by induction the serial parser passes
 * through every position the index names.  Whatever fails sends the frame down the serial route from the start.
 *
 * mpc_container_index: host only, no context, safe on several threads: one serial parse that records the positions.  interval:
 * coded symbols per checkpoint, 32 ... 65536, 0 = the library's default.  index: flat, little-endian, versioned
 * (layout in DESIGN.md), release with mpc_free.  MPC_ERR_BITSTREAM for whatever mpc_read_compressed_coded refuses.  A container
 * with a Huffman table of codes longer than 32 bits (no encoder writes one) gets a valid index that says "serial only". */
mpc_status mpc_container_index(const uint8_t* bytes, size_t nbytes, int interval, uint8_t** index, size_t* index_bytes);
typedef struct mpc_index_header {
    int interval, n_streams;        /* n_streams = 1 + 6K, the lengths stream first */
    int serial_only;                /* 1: no checkpoints; every decode with this index takes the serial route */
    int width, height, K, block_size;
    size_t container_bytes;
} mpc_index_header;
typedef struct mpc_index_stream_info {
    int mode;                       /* 0 Huffman, 1 Golomb */
    int packed;                     /* the container's run-length flag */
    uint32_t m;                     /* Golomb parameter */
    uint64_t n_coded;               /* symbols the entropy decode yields */
    uint64_t expect;                /* symbols the stream expands to */
    uint64_t wrapper_bit;           /* where the stream's wrapper begins: run-length flag, packed size, Huffman/Golomb bit, table or M */
    uint64_t end_bit;               /* behind its last bit (behind the pseudo-EOF for Huffman) = the next stream's wrapper_bit */
    uint64_t n_checkpoints;         /* ceil(n_coded / interval); checkpoint j = the bit of coded symbol j * interval */
} mpc_index_stream_info;
/* An index read back (its own consistency only; nothing is said about any container): MPC_ERR_BITSTREAM if it is not one.
 * checkpoints: NULL, or room for `capacity` >= n_checkpoints values. */
mpc_status mpc_index_info(const uint8_t* index, size_t index_bytes, mpc_index_header* info);
mpc_status mpc_index_stream(const uint8_t* index, size_t index_bytes, int stream, mpc_index_stream_info* info, uint64_t* checkpoints,
                            size_t capacity);
/* Index version 2 ("expanded"): the version-1 blob with its version word set to 2, followed by an aux section that lets a region
 * decode cut the streams version 1 cannot cut -- a run-length packed stream (coded positions are not expanded positions) and the
 * three step-0 coefficient streams 1, 2K + 1, 4K + 1 (prefix sums).  Only those streams have entries (which they are follows
 * from the stream records: `packed`, or a step-0 coefficient stream; the lengths stream has none).  Section: u64 entries in all,
 * then, stream behind stream in the blob's order, 16 bytes per checkpoint j (coded symbol j * interval) of each such stream:
 *   u64 out    expanded symbols emitted by the coded symbols [0, j * interval) under runLengthDecode's machine; j * interval
 *              for a stream that is not packed
 *   u64 word   bits 0-15 prev: coded symbol j * interval - 1 (0 for j = 0 and for a stream that is not packed); bits 16-31 dc:
 *              for a step-0 coefficient stream the low 16 bits of the sum of zigzagDecode over those `out` expanded symbols, else
 *              0; bits 32-33 state: the machine's state coded symbol j * interval is met in (0 fresh, 1 value, 2 count; 0 for a
 *              stream that is not packed); the other bits 0
 * A "serial only" index has no entries.  The blob is a pure function of (container, interval).  Every call that takes an index
 * takes either version; whole-frame decodes and MPC_REGION_PARSE_ALL check the section's structure and use nothing else of it.
 *
 * mpc_container_index2: flags 0 = mpc_container_index's blob, byte for byte; MPC_INDEX_EXPANDED = version 2 (one more linear pass
 * over the packed and step-0 streams).  Refusals are mpc_container_index's.
 * mpc_index_extend: from the version-1 index of this container (what the indexed encoders return) the version-2 blob
 * mpc_container_index2 would build with that index's interval, byte for byte, without the serial parse: the streams come from the
 * chunked parse.  An index that is refused is answered from the serial parse, with the interval its header word names (the
 * default where that is none).  A version-2 index comes back as a copy.  MPC_ERR_BITSTREAM for a container
 * mpc_read_compressed_coded refuses.
 * mpc_index_version: 1 or 2; 0 = not an index.
 * mpc_index_aux: a stream's entries read back; *n_entries = 0 for a version-1 index and for a stream without entries.  out, prev,
 * state, dc: each NULL or room for `capacity` >= *n_entries values (all NULL: the count alone). */
#define MPC_INDEX_EXPANDED 1u
mpc_status mpc_container_index2(const uint8_t* bytes, size_t nbytes, int interval, unsigned flags, uint8_t** index, size_t* index_bytes);
mpc_status mpc_index_extend(const uint8_t* bytes, size_t nbytes, const uint8_t* index_v1, size_t index_v1_bytes, uint8_t** index,
                            size_t* index_bytes);
int mpc_index_version(const uint8_t* index, size_t index_bytes);
mpc_status mpc_index_aux(const uint8_t* index, size_t index_bytes, int stream, uint64_t* out, uint16_t* prev, uint8_t* state, uint16_t* dc,
                         size_t capacity, size_t* n_entries);
/* The seek index without a serial parse of the container ("Seek index from a bit scan").  Which code begins at
 * bit p of a stream and how long it is depends on the bits at p and the stream's table alone; evaluated at every bit of a window,
 * the serial parse is a walk along p -> p + len(p) that composes segment by segment.  Per stream, in container order: a step table
 * over a window of `window_bits` behind the stream's first code, a map per segment of `segment_bits` (from every bit the first code
 * start at or behind the segment's end and the codes on the way), the chain of those maps from the first code, and a walk of every
 * segment from its true entry that writes the checkpoints; a stream longer than a window continues in the next from the carried
 * (position, ordinal).  The host reads each wrapper in between; the sizes of streams 1 ... 6K come from the lengths stream, decoded
 * from its fresh checkpoints.
 * mpc_container_index_scan: that on the host, with no context -- it defines what the device scan computes.  Status, error text and
 * blob are mpc_container_index2's, byte for byte, for every input.  *route: 0 = the scan produced the blob; 1 = the scan gave up
 * (a wrapper the reader refuses, a Huffman table deeper than 32 bits, a dead chain, a count or size the serial parser would not
 * accept, a Golomb unary run of 65536 bits or more) and the serial builder produced the result or the refusal.  A proposed blob is
 * reported on route 0 only once the acceptance rule above has passed it (then it is the serial parser's path), and the scan does
 * not give up on a container whose serially built index mpc_parse_container_by_index uses.  segment_bits, window_bits: 0 = the
 * library's defaults (256 and 2^22); else, for tests, a segment of 32 ... 32768 bits and a window of whole segments of at most
 * 2^26 bits; anything else MPC_ERR_ARGUMENT.
 * mpc_container_index_device: the same contract with the step table, the maps, the chain and the walk on the device (mp_scan.hip)
 * and the acceptance by the device parse; route 1 = the host builder ran.
 * mpc_debug_container_index_device: mpc_container_index_device (flags 0) with the sizes given, for tests.
 * mpc_decode_images_scan[_device]: mpc_decode_images[_device] for frames that come without an index: per frame the device scan, then
 * the indexed route with the proposed index.  Pixels, statuses and error texts are those of mpc_decode_images[_device].  routes:
 * NULL, or per frame 0 = scanned and parsed on the device, 1 = the serial route (the scan gave up or the device refused the index).
 * indexes: NULL, or per frame the version-1 blob of a frame on route 0 (mpc_free; a cache can keep it), NULL with size 0 for a
 * frame on route 1; index_bytes goes with it. */
mpc_status mpc_container_index_scan(const uint8_t* bytes, size_t nbytes, int interval, unsigned flags, int segment_bits, int window_bits,
                                    uint8_t** index, size_t* index_bytes, int* route);
mpc_status mpc_container_index_device(mpc_context* ctx, const uint8_t* bytes, size_t nbytes, int interval, unsigned flags, uint8_t** index,
                                      size_t* index_bytes, int* route);
mpc_status mpc_debug_container_index_device(mpc_context* ctx, const uint8_t* bytes, size_t nbytes, int interval, int segment_bits,
                                            int window_bits, uint8_t** index, size_t* index_bytes, int* route);
mpc_status mpc_decode_images_scan(mpc_context* ctx, const uint8_t* const* bytes, const size_t* nbytes, int n_frames, uint8_t** rgb,
                                  int* width, int* height, uint8_t** indexes, size_t* index_bytes, int* routes);
mpc_status mpc_decode_images_scan_device(mpc_context* ctx, const uint8_t* const* bytes, const size_t* nbytes, int n_frames,
                                         uint8_t* const* d_rgb, const size_t* capacity, int* width, int* height, uint8_t** indexes,
                                         size_t* index_bytes, int* routes);
/* The indexed encoders with `flags`, in the way mpc_container_index2 extends mpc_container_index: the arguments of
 * mpc_encode_images_indexed[_device], mpc_code_symbol_streams_device_indexed and mpc_assemble_symbol_streams_by_plan_indexed with
 * `flags` behind `interval`.
 *   flags == 0                   exactly that call: the same containers, the version-1 blobs, the same kernels
 *   flags == MPC_INDEX_EXPANDED  indexes[i] is the blob mpc_container_index2(bytes[i], nbytes[i], interval, MPC_INDEX_EXPANDED, ...)
 *                                returns, byte for byte; the containers are those of the calls without an index
 *   any other bit                MPC_ERR_ARGUMENT before anything is enqueued
 * The aux entries come from the device's entropy stage too, so a region or view decode can follow the encode with no pass over the
 * container on the host (mpc_index_extend) in between: the kernel that writes a run-length packed stream holds, at every symbol it
 * writes, the expanded position, the symbol in front and the state the decoder will be in, and stores them at every interval-th;
 * the sums of the step-0 coefficient streams are prefix sums over streams the stage holds.  The host checks the entries against
 * its plans (an entry per checkpoint, out[0] = 0, strictly increasing, inside the stream, a state that exists, c * interval for a
 * stream that is not packed) and builds the blob from the finished container instead where they do not hold; a frame whose
 * entropy stage takes the host route gets it that way as well.  The by-plan form computes the entries on the host from the coded
 * streams it holds and so defines, without a GPU, what the device computes.  Interval rules, the single-frame route, mpc_free, no
 * result on failure, and no index (and no error) for streams that do not hold what `counts` implies: as for the calls without
 * `flags`. */
mpc_status mpc_encode_images_indexed2(mpc_context* ctx, const uint8_t* const* rgb_frames, int n_frames, int width, int height,
                                      const double* quant, int interval, unsigned flags, uint8_t** bytes, size_t* nbytes,
                                      uint8_t** indexes, size_t* index_bytes);
mpc_status mpc_encode_images_indexed2_device(mpc_context* ctx, const uint8_t* const* d_rgb_frames, int n_frames, int width, int height,
                                             const double* quant, int interval, unsigned flags, uint8_t** bytes, size_t* nbytes,
                                             uint8_t** indexes, size_t* index_bytes);
mpc_status mpc_code_symbol_streams_device_indexed2(mpc_context* ctx, int width, int height, const double* quant, const uint16_t* counts,
                                                   const uint16_t* symbols, const unsigned long long* stream_off, int interval,
                                                   unsigned flags, uint8_t** bytes, size_t* nbytes, uint8_t** index, size_t* index_bytes,
                                                   int* route);
mpc_status mpc_assemble_symbol_streams_by_plan_indexed2(int width, int height, int K, int block_size, const double* quant,
                                                        const uint16_t* counts, const uint16_t* symbols,
                                                        const unsigned long long* stream_off, int interval, unsigned flags,
                                                        uint8_t** bytes, size_t* nbytes, uint8_t** index, size_t* index_bytes);
/* The chunked parse on the host: what mpc_read_compressed_coded yields -- the lengths stream and the 6K coded streams back to back
 * (symbols, mpc_free) -- with every chunk decoded from its checkpoint alone and accepted only under the rule above.  It defines
 * what the device parse computes, checkable without a GPU.  route: 0 = the index was used, 1 = it was refused and the serial
 * parse produced the result.  Status and text are mpc_read_compressed_coded's. */
mpc_status mpc_parse_container_by_index(const uint8_t* bytes, size_t nbytes, const uint8_t* index, size_t index_bytes,
                                        uint16_t** symbols, size_t* n_symbols, int* route);
/* The same on the device (mp_parse.hip), for tests: the decoder's own upload-and-parse step with host buffers in and out. */
mpc_status mpc_parse_container_device(mpc_context* ctx, const uint8_t* bytes, size_t nbytes, const uint8_t* index, size_t index_bytes,
                                      uint16_t** symbols, size_t* n_symbols, int* route);
/* mpc_decode_images / mpc_decode_images_device with an optional index per frame: indexes[f] == NULL (or indexes == NULL) = the
 * serial route for frame f.  A frame with an index uploads the container's bytes instead of its parsed streams and has its
 * entropy codes parsed by the device.  routes: NULL, or per frame 0 = parsed on the device, 1 = serial (no index, or the index
 * was refused).  Pixels, statuses and error texts are those of the calls without indexes.  As with those calls, the content of
 * d_rgb[f] after a call that failed is unspecified (a frame whose index the device refused has been written once before the
 * serial route decides about it). */
mpc_status mpc_decode_images_indexed(mpc_context* ctx, const uint8_t* const* bytes, const size_t* nbytes, const uint8_t* const* indexes,
                                     const size_t* index_bytes, int n_frames, uint8_t** rgb, int* width, int* height, int* routes);
mpc_status mpc_decode_images_indexed_device(mpc_context* ctx, const uint8_t* const* bytes, const size_t* nbytes,
                                            const uint8_t* const* indexes, const size_t* index_bytes, int n_frames, uint8_t* const* d_rgb,
                                            const size_t* capacity, int* width, int* height, int* routes);

/* ---- a pixel rectangle of a frame through its seek index ("Decoder: regions") ----
 * What a viewer or a cache of compressed frames asks for: rects[f] of frame f instead of the whole frame.  rgb[f] (mpc_free) /
 * d_rgb[f] receive rects[f].height x rects[f].width x 3 bytes, tightly packed; capacity[f] must be at least that, and bytes behind
 * it are untouched.  A rectangle that is empty or not inside the frame's own width and height is MPC_ERR_ARGUMENT, reported
 * before anything is enqueued ("frame N: ..."); so is a capacity too small for it.
 *
 * The window.  The 6K streams are compactions of the records in tile order, column-major (t = tx * tiles_y + ty).  For a
 * rectangle (x, y, w, h): tx0 = x / 8, tx1 = ceil((x + w) / 8), ty0 = y / 8, ty1 = ceil((y + h) / 8); its tiles, the grid
 * [tx0, tx1) x [ty0, ty1), lie in the one contiguous range [t0, t1) = [tx0 * tiles_y + ty0, (tx1 - 1) * tiles_y + ty1), and that
 * range owns the positions [r0, r1) of the stream pair (channel, step): r = the tiles in front whose length, cut to K, exceeds the
 * step.  The lengths stream (3 symbols a tile) is parsed whole and gives every r; of a stream that is neither run-length packed
 * nor difference coded only the chunks [r0 / interval, ceil(r1 / interval)) are parsed, and everything behind the parse -- the
 * copy of unpacked streams, the gather, the reconstruction, the pixels' way back -- handles the window alone.
 * The cost follows the rectangle's HORIZONTAL extent: [t0, t1) spans every tile column the rectangle touches from top to bottom
 * (but for the first and last), so a wide, short strip spans nearly every column's whole range; ranges per tile column are not
 * built.  A run-length packed stream (coded positions are not expanded positions) and the three step-0 coefficient streams
 * (prefix sums) are cut through a version-2 index: with out[], state[], prev[], dc[] of the stream's aux entries, c0 = the largest
 * j with out[j] <= r0, c1 = the smallest j > c0 with out[j] >= r1, else the stream's chunks (r0 == r1: nothing is parsed).  Only
 * chunks [c0, c1) are parsed; the expansion starts at coded symbol c0 * interval in (state[c0], prev[c0]) at position out[c0], the
 * sum seeded with dc[c0].  With a version-1 index, and under MPC_REGION_PARSE_ALL, those streams are parsed and expanded whole.
 *
 * What is trusted.  Without MPC_REGION_PARSE_ALL the chunks outside the window are never read, so the whole-frame rule "a hint,
 * never an authority" cannot hold in full.  What holds instead: (1) every structural check of the whole-frame route is kept --
 * the index against the container on the host, the aux section's structure included (its size exact; per stream out[0] = 0,
 * state[0] = 0, prev[0] = 0, out strictly increasing and <= expect, state <= 2, out[j] = j * interval for a stream that is not
 * packed); the lengths stream parsed whole, and with a version-1 index every packed stream and the three step-0 coefficient
 * streams too, checked as for a whole frame; the stream sizes recomputed from the decoded lengths equal to the index's; every
 * parsed chunk yielding exactly its symbols and ending on the next checkpoint (on the pseudo-EOF and the stream's end for a last
 * chunk); for a stream cut through its aux entries, behind the last parsed coded symbol the expansion's position and state equal
 * to out[c1] and state[c1], that symbol equal to prev[c1] and the running sum to dc[c1] (c1 = the stream's chunks: the position
 * equal to `expect`, a dangling count dropped) -- checked before anything of the stream is written.  Any failure sends the frame
 * to route 1.  (2) With an index that mpc_container_index[2], mpc_index_extend or the indexed encoders made for this container
 * the result is exactly the crop of the full decode; with any other index that passes all of (1) -- checkpoints or aux entries
 * that were not made for this container -- the pixels are unspecified.  Nothing is read or written out of bounds either way:
 * every bound still comes from the host's tables and the checked aux entries (out <= expect), never from a symbol's value.
 * With MPC_REGION_PARSE_ALL every chunk of every stream is parsed, the whole-frame acceptance rule applies unchanged, and only
 * the stages behind the parse are windowed.  In either mode the reconstruction's "Invalid bitstream" verdict (a record outside
 * its dictionary) speaks for the window's tiles only.
 *
 * routes (NULL, or per frame): 0 = windowed; 1 = the whole frame decoded by the serial route into the decode slot's own device
 * memory and cropped by a 2-D copy -- no index (indexes == NULL or indexes[f] == NULL), a refused index, "serial only".  Route 1
 * exists so that the call always answers; statuses and texts of a frame that does not decode are those of mpc_decode_images. */
typedef struct mpc_rect { int x, y, width, height; } mpc_rect;
#define MPC_REGION_PARSE_ALL 1u
mpc_status mpc_decode_regions_indexed(mpc_context* ctx, const uint8_t* const* bytes, const size_t* nbytes, const uint8_t* const* indexes,
                                      const size_t* index_bytes, const mpc_rect* rects, int n_frames, unsigned flags, uint8_t** rgb,
                                      int* routes);
mpc_status mpc_decode_regions_indexed_device(mpc_context* ctx, const uint8_t* const* bytes, const size_t* nbytes,
                                             const uint8_t* const* indexes, const size_t* index_bytes, const mpc_rect* rects, int n_frames,
                                             unsigned flags, uint8_t* const* d_rgb, const size_t* capacity, int* routes);
/* The windowed parse on the host, the role mpc_parse_container_by_index plays for the whole frame: the same plan, the same chunk
 * decoders and the same acceptance as the device route, checkable without a GPU.  symbols (mpc_free): the lengths whole, then for
 * each of the 6K streams its EXPANDED symbols [r0, r1) back to back -- run lengths undone, step-0 coefficients summed: a slice of
 * the whole-frame expansion whichever streams were cut.  ranges[3K][2]: (r0, r1) of every (channel, step) pair.  route as above
 * (1: mpc_read_compressed gave the result).  MPC_ERR_BITSTREAM for a container mpc_read_compressed refuses, MPC_ERR_ARGUMENT for
 * a rectangle that is empty or not inside the frame. */
mpc_status mpc_parse_container_window_by_index(const uint8_t* bytes, size_t nbytes, const uint8_t* index, size_t index_bytes,
                                               const mpc_rect* rect, unsigned flags, uint16_t** symbols, size_t* n_symbols,
                                               uint64_t* ranges, int* route);
/* The device half (upload, lengths parse, rank, windowed parse, windowed unpack), for tests: host buffers in and out. */
mpc_status mpc_parse_container_window_device(mpc_context* ctx, const uint8_t* bytes, size_t nbytes, const uint8_t* index,
                                             size_t index_bytes, const mpc_rect* rect, unsigned flags, uint16_t** symbols,
                                             size_t* n_symbols, uint64_t* ranges, int* route);
/* The chunks [chunks[i][0], chunks[i][1]) of each of the 6K streams that the windowed parse reads for this rectangle (all of a
 * stream's chunks where it is parsed whole).  Host only; needs the lengths stream alone.  route 1 (the index is refused, or the
 * lengths are not what it says): no chunk is parsed by index, every entry 0.  The _device form (for tests) runs the upload, the
 * lengths parse and mp_window_rank_kernel, nothing behind it, and downloads the device's own table; where the device's lengths
 * parse sets its error word the answer is the host's route 1. */
mpc_status mpc_window_chunks_by_index(const uint8_t* bytes, size_t nbytes, const uint8_t* index, size_t index_bytes, const mpc_rect* rect,
                                      unsigned flags, uint64_t* chunks /* [6K][2] */, int* route);
mpc_status mpc_window_chunks_device(mpc_context* ctx, const uint8_t* bytes, size_t nbytes, const uint8_t* index, size_t index_bytes,
                                    const mpc_rect* rect, unsigned flags, uint64_t* chunks /* [6K][2] */, int* route);

/* ---- views: the first n steps, reduced 2/4/8x, of a frame or a rectangle of it ("Decoder: views") ----
 * The container is layered by pursuit step: stream 1 + 2K*ch + 2i and the one behind it hold step i of every tile-channel that has
 * it, and a tile-channel has step i exactly when its length exceeds i.
 *
 * mpc_truncate_container: the container of the same frame cut to its first `steps` steps -- the product's rate-scalable transcode
 * (a lower-rate file without encoding again).  Host only, no context.  The input is parsed with mpc_read_compressed; every length
 * becomes min(length, steps); the streams of steps below `steps` are kept (the same symbols), those of steps at or above it are
 * emptied; header, K and the quantiser table are kept; the result is written by the one host coder.  steps >= K: a copy of what
 * coding the parsed container again gives, for an encoder's container the input itself.  steps < 1: MPC_ERR_ARGUMENT.  Whatever
 * mpc_read_compressed refuses: MPC_ERR_BITSTREAM.  out: mpc_free.  (The kept streams are unchanged as symbols for whatever an encoder
 * writes.  A damaged container whose step-0 coefficient sums move by 2^15 or more from tile to tile is not: the difference coder keeps
 * 16 bits of a 17-bit zig-zag code, in the reference's writer as here.  A view reads such sums as the decoder does.)
 *
 * A view of a frame is a rectangle of it, reconstructed from the first `steps` records of every tile-channel and reduced by
 * c = 2^scale_log2:
 *   steps       0 = all; < 0 is MPC_ERR_ARGUMENT; above the container's K acts as K.  The pixels, statuses and error texts of a view
 *               with steps = m are those of a decode of mpc_truncate_container(m): a tile-channel's dynamic dictionary is built from
 *               its first m choices only, so a record outside the dictionary at a step at or above m no longer refuses, and a record
 *               below m whose block only a step at or above m unlocks does ("Invalid bitstream").
 *   scale_log2  0 ... 3, else MPC_ERR_ARGUMENT; rect.x and rect.y must be multiples of c (else MPC_ERR_ARGUMENT), width and height
 *               are free.  The output is ceil(height / c) rows of ceil(width / c) pixels x 3 bytes, tightly packed.  Output pixel
 *               (i, j) covers the full-resolution pixels of the cell [x + i*c, x + (i+1)*c) x [y + j*c, y + (j+1)*c) that lie inside
 *               the rectangle, n of them, 1 <= n <= c*c; per colour channel its value is (sum + n/2) / n in integers over the STORED
 *               8-bit values (after RGBFromYUV's rounding and clamp).
 *   rect        width == 0 && height == 0 with x = y = 0: the whole frame; otherwise the rules of mpc_decode_regions_indexed.
 * A view with steps = 0 and scale_log2 = 0 equals mpc_decode_regions_indexed of the same rectangle, pixel for pixel.
 * width[f] / height[f] receive the output's size.  A capacity below 3 * ceil(w / c) * ceil(h / c) is MPC_ERR_ARGUMENT, reported before
 * anything is enqueued ("frame N: ..."), as are the argument errors above and a rectangle outside the frame.
 *
 * Routes.  0 needs a usable index of version 1 or 2 and runs the region decoder's order (see above) with every stream of a step at
 * or above `steps` given an empty chunk range: it is neither parsed, unpacked nor gathered.  The lengths stream is parsed whole and
 * the stream sizes recomputed from the UNCUT lengths are compared with the index's; only behind that check are the lengths cut (on
 * the device, in place), and the host's stream tables hold the cut streams empty, so every bound still comes from the host's
 * tables, never from a symbol's value.  1 (no index, a refused index, "serial only"): the serial parse of the whole container, the
 * lengths and streams cut on the host as the truncation cuts them (a cut stream is first held to the size the lengths give it, as
 * mpc_read_compressed holds it), then the ordinary upload, unpack and gather and the same reconstruction: no full-size frame exists
 * on either route.
 *
 * What is trusted.  Without MPC_VIEW_PARSE_ALL the statement of the regions section holds, extended by "streams of steps >= steps":
 * like the chunks outside the window they are never read on route 0, so a container damaged only there still yields its view.
 * With MPC_VIEW_PARSE_ALL every chunk of every stream is parsed and every packed stream expanded, the whole-frame acceptance rule
 * applies unchanged, and only the stages behind the parse are windowed and cut. */
typedef struct mpc_view { mpc_rect rect; int steps; int scale_log2; } mpc_view;
#define MPC_VIEW_PARSE_ALL 1u
mpc_status mpc_truncate_container(const uint8_t* bytes, size_t nbytes, int steps, uint8_t** out, size_t* out_bytes);
mpc_status mpc_decode_views_indexed(mpc_context* ctx, const uint8_t* const* bytes, const size_t* nbytes, const uint8_t* const* indexes,
                                    const size_t* index_bytes, const mpc_view* views, int n_frames, unsigned flags, uint8_t** rgb,
                                    int* width, int* height, int* routes);
mpc_status mpc_decode_views_indexed_device(mpc_context* ctx, const uint8_t* const* bytes, const size_t* nbytes,
                                           const uint8_t* const* indexes, const size_t* index_bytes, const mpc_view* views, int n_frames,
                                           unsigned flags, uint8_t* const* d_rgb, const size_t* capacity, int* width, int* height,
                                           int* routes);
/* The host definition of the device parse of a view, the role mpc_parse_container_window_by_index plays for regions: by
 * construction the windowed parse of the truncated container, from this container and its own index.  symbols (mpc_free): the
 * lengths CUT to `steps`, then for each of the 6K streams its expanded symbols [r0, r1) of the window; a stream of a step at or
 * above `steps` is empty, r0 = r1 = 0.  ranges[3K][2], route, statuses as for mpc_parse_container_window_by_index;
 * view->scale_log2 is checked and otherwise unused. */
mpc_status mpc_parse_container_view_by_index(const uint8_t* bytes, size_t nbytes, const uint8_t* index, size_t index_bytes,
                                             const mpc_view* view, unsigned flags, uint16_t** symbols, size_t* n_symbols,
                                             uint64_t* ranges, int* route);
/* The device half (upload, lengths parse, lengths cut, rank, windowed parse, windowed unpack), for tests: host buffers in and out. */
mpc_status mpc_parse_container_view_device(mpc_context* ctx, const uint8_t* bytes, size_t nbytes, const uint8_t* index,
                                           size_t index_bytes, const mpc_view* view, unsigned flags, uint16_t** symbols,
                                           size_t* n_symbols, uint64_t* ranges, int* route);

/* ---- transcode: a view of a container as a container ("Transcode") ----
 * A tile's records depend on that tile's pixels alone, the 6K streams are compactions of the records in tile order, and the step-0
 * difference coding is a function of that order: for a tile-aligned rectangle the container of the cropped image is a pure function of
 * the source container's symbols.  No pixels, no pursuit, no second loss.
 *
 * mpc_transcode_container: host only, no context; it defines what the device route computes.
 *   input       parsed with mpc_read_compressed; what that refuses is MPC_ERR_BITSTREAM "Invalid input data"; a length above K anywhere
 *               in the frame is MPC_ERR_BITSTREAM "Invalid bitstream".
 *   scale_log2  must be 0, else MPC_ERR_ARGUMENT.
 *   steps       the views' rule: 0 = all, < 0 is MPC_ERR_ARGUMENT, above K acts as K.  Call the result m.
 *   rect        (0, 0, 0, 0): the whole frame.  Otherwise non-empty and inside the frame (the region decoder's checks), and aligned to
 *               the container's own block size b (1 ... 8 on the host): x % b == 0, y % b == 0, x + width a multiple of b or the frame's
 *               width, y + height a multiple of b or the frame's height; anything else is MPC_ERR_ARGUMENT.  A ragged right or bottom
 *               edge is legal only where it is the frame's own: there the zero fill of a fresh encode of the crop is the source's.
 *   result      (mpc_free) the container of width x height of the rectangle with the source's K, block size and 3K u16 quantiser
 *               values.  Tile t' = (tx - tx0) * nty + (ty - ty0) of the new frame, nty = ty1 - ty0, takes the records of tile
 *               t = tx * tiles_y + ty of the source; its lengths are min(length, m), records of steps >= m are dropped.  The streams are
 *               assembled in the new tile order and written by the one host coder: step-0 coefficients are difference coded again from
 *               zero, packed-or-not and Huffman-or-Golomb are chosen again.
 * No dictionary is involved: a record outside its dynamic dictionary is carried over as it is, and a decoder refuses the result
 * exactly where it would have refused those tiles of the source.  mpc_truncate_container's caveat holds here too: step-0 sums that move
 * by 2^15 or more from tile to tile (no encoder writes them) are not kept by the difference coder.
 * Consequences: the whole frame with steps 0 is a copy of what coding the parsed container again gives, for an encoder's container
 * the input itself; the whole frame with steps m is mpc_truncate_container(m); transcodes compose (a rectangle of a rectangle is
 * the rectangle of the source, and cutting steps commutes with cropping); and for a container an encoder made from pixels P with
 * quantiser tables q the result is byte for byte mpc_truncate_container(mpc_encode_image(crop of P, q), m).
 *
 * mpc_transcode_views_indexed: the same bytes, statuses and error texts per frame from the device (refusals carry "frame N: ").
 * out[f] (mpc_free) / out_bytes[f]: frame f's container.  routes as for the views.
 *   route 0     needs a usable index, version 1 or 2: the view decoder's order up to the gather (upload, lengths parsed whole, ranks,
 *               the windowed parse with the streams of steps >= m given empty chunk ranges, the windowed unpack, the windowed gather),
 *               then mp_crop_records_kernel and the records-to-container chain (stream assembly, entropy phase 1, host tables, phase 2,
 *               the copy) instead of the reconstruction.  MPC_VIEW_PARSE_ALL and what is trusted without it are the views', word for
 *               word: without the flag, chunks outside the window and streams of steps >= m are never read.
 *   route 1     no index, a refused index, "serial only": the serial parse on the host, cut as the truncation cuts it, the ordinary
 *               upload, unpack and whole-frame gather, then the same crop kernel and the same chain.  No pixels exist on either route.
 * The container's block size must be the context's, as for the decoders, and its K must be mpc_context_K(ctx), else MPC_ERR_ARGUMENT
 * (both reported behind mpc_read_compressed's verdict); a host-only context is MPC_ERR_NO_DEVICE; the fast flag changes nothing.  The
 * header's u16 quantiser values are passed on as doubles and truncated back to the same values.  The call runs on the context's
 * container job slots: all of them must be idle (else MPC_ERR_ARGUMENT), and they are left idle.  On failure nothing is returned:
 * every out[f] is NULL, every size 0, and the context is usable.  Frames of a call overlap on the decode slots; a result depends
 * neither on n_frames nor on the order of the frames. */
mpc_status mpc_transcode_container(const uint8_t* bytes, size_t nbytes, const mpc_view* view, uint8_t** out, size_t* out_bytes);
mpc_status mpc_transcode_views_indexed(mpc_context* ctx, const uint8_t* const* bytes, const size_t* nbytes, const uint8_t* const* indexes,
                                       const size_t* index_bytes, const mpc_view* views, int n_frames, unsigned flags, uint8_t** out,
                                       size_t* out_bytes, int* routes);
/* The crop kernel on the caller's records, e.g. those of mpc_encode_tiles_device for tile rows [0, tiles_y): several containers cut out
 * of one pursuit (mpc_records_to_container_device of the result with the rectangle's width and height).  Whole-frame records of a
 * width x height frame (tile t = tx * tiles_y + ty, counts[t * 3 + ch], choices[(t * 3 + ch) * K + i], K the context's) in; rect as for
 * mpc_transcode_container with b the context's block size; steps 0 = all.  d_out_counts[tiles' * 3], d_out_choices[tiles' * 3 * K] of the
 * rectangle's tiles' = ntx * nty: counts min(count, steps), the records below that copied, the steps from there to K zero.  Asynchronous
 * on `stream`; the outputs must not overlap the inputs.  Every address comes from the rectangle's tile grid; a count above K is used as
 * K and sets the context's crop error word, which mpc_crop_records_check(ctx, stream) reads and clears behind everything enqueued on
 * `stream` (it synchronises the stream): MPC_ERR_BITSTREAM "Invalid bitstream" if a crop since the last check saw one, else MPC_OK. */
mpc_status mpc_crop_records_device(mpc_context* ctx, const uint16_t* d_counts, const mpc_basis_choice* d_choices, int width, int height,
                                   const mpc_rect* rect, int steps, uint16_t* d_out_counts, mpc_basis_choice* d_out_choices, void* stream);
mpc_status mpc_crop_records_check(mpc_context* ctx, void* stream);

/* ---- compose: a container from rectangles of containers and pixels ("Compose") ----
 * The inverse of the transcode, from the same two facts: the container of an image assembled from tile-aligned pieces is a pure function
 * of the pieces' records.  Untouched tiles see no pixel, no pursuit and no second loss.
 *
 * mpc_compose_container: host only, no context; it defines what the device route computes.  The result (mpc_free) is the container of a
 * width x height frame with the K, block size b and 3K u16 quantiser values of source 0.  Parts are applied in order and a later part
 * wins a tile: a tile's OWNER is the last part whose destination grid holds it, and destination tile (dtx0 + i) * tiles_y + (dty0 + j)
 * takes the counts and records of the owner's source tile (stx0 + i) * src_tiles_y + (sty0 + j).  The streams are assembled in the
 * destination's tile order and written by the one host coder: step-0 sums are difference coded from zero again, packed-or-not and
 * Huffman-or-Golomb are chosen again.  No dictionary is involved, and mpc_truncate_container's caveat about step-0 sums that move by
 * 2^15 or more from tile to tile is inherited.  Checks, in this order, the first failure wins:
 *   1. arguments that need no container, MPC_ERR_ARGUMENT: null pointers, n_parts < 1, width or height < 1, n_sources < 0, a `source`
 *      outside [-1, n_sources), a pixel part ("part N: pixels need a device": the host computes no tiles), n_sources == 0.
 *   2. every source's header, named by a part or not: what the header parse of mpc_container_info refuses is MPC_ERR_BITSTREAM
 *      "source N: Invalid input data"; a K, block size or one of the 3K u16 quantiser values that is not source 0's is MPC_ERR_ARGUMENT
 *      "source N: ...".  A container holds one quantiser table.
 *   3. every part's geometry, MPC_ERR_ARGUMENT "part N: ...": rect passes mpc_transcode_container's checks on its source; x % b == 0,
 *      y % b == 0, x + w <= width, y + h <= height (in 64 bits); and per axis the rectangle's far edge is a multiple of b, or it is the
 *      source frame's own ragged edge AND lands on the destination's own edge (x + w == width).  A ragged tile carries its zero fill and
 *      is the encode of pasted pixels only where the destination is ragged in the same way.
 *   4. coverage: every destination tile has an owner, else MPC_ERR_ARGUMENT naming the first uncovered tile in tile order.
 *   5. every source that an OWNING part names is parsed with mpc_read_compressed: what that refuses is MPC_ERR_BITSTREAM "part N: Invalid
 *      input data", a length above K anywhere in the source "part N: Invalid bitstream", N the lowest failing owning part.  A part that
 *      owns no tile is not read beyond its header: a body damaged only there changes nothing.
 * Consequences: one whole-frame part is what coding the parsed container again gives, for an encoder's container the input itself;
 * composing the tile-aligned pieces of a source that mpc_transcode_container cut gives the source; compose and transcode commute (a
 * rectangle of a composition is the composition of the rectangles); and containers encoded from pixels with one integral quantiser
 * table (those of mpc_quant_tables are integral) give, byte for byte, mpc_encode_image of the pasted pixels. */
typedef struct mpc_part {
    int source;          /* >= 0: bytes[source] is a container and `rect` a rectangle of it, (0,0,0,0) = all of it;  -1: pixels */
    mpc_rect rect;       /* source == -1: x = y = 0, width x height of the pixels */
    int x, y;            /* where the rectangle's top-left lands in the destination */
    const uint8_t* rgb;  /* source == -1 only: pixel (i, j) is the 3 bytes at rgb + j * row_stride + 3 * i */
    size_t row_stride;   /* 0 = 3 * width, else >= 3 * width */
} mpc_part;
mpc_status mpc_compose_container(const uint8_t* const* bytes, const size_t* nbytes, int n_sources, const mpc_part* parts, int n_parts,
                                 int width, int height, uint8_t** out, size_t* out_bytes);
/* The paste kernel (mp_paste_records_kernel) on the caller's records.  Both sides are whole-frame records (t = tx * tiles_y + ty,
 * counts[t * 3 + ch], choices[(t * 3 + ch) * K + i], K the context's).  For every tile of src_rect's grid ((0,0,0,0) = the whole source)
 * the destination tile at the same offset from (dst_x, dst_y) gets its three counts and 3K record words: records below the count are
 * copied, the steps from the count to K are written as zero, so garbage behind a source count is never carried over.  d_owner: NULL, or
 * one int32 per destination tile in destination order; a tile is then written only where d_owner[t] == part.  Everything else in the
 * destination stays as it was.  The geometry rules are those of check 3 above with b the context's block size, checked on the host
 * before anything is enqueued; every address comes from the two grids, never from a record.  A count above K is used as K and sets the
 * context's crop error word (mpc_crop_records_check reads and clears it).  Asynchronous on `stream`; source and destination must not
 * overlap.  Pastes that share an owner map write disjoint tiles: they may run on different streams in any order. */
mpc_status mpc_paste_records_device(mpc_context* ctx, const uint16_t* d_src_counts, const mpc_basis_choice* d_src_choices, int src_width,
                                    int src_height, const mpc_rect* src_rect, uint16_t* d_dst_counts, mpc_basis_choice* d_dst_choices,
                                    int dst_width, int dst_height, int dst_x, int dst_y, const int32_t* d_owner, int part, void* stream);
/* mpc_compose_indexed: the bytes, statuses and error texts of mpc_compose_container from the device, in which every pixel part stands
 * for "the container this context's mpc_encode_image makes of those pixels with the destination's quantiser table".  indexes /
 * index_bytes are per source; an entry or the whole array may be NULL.  The quantiser table is source 0's u16 values as doubles; with
 * n_sources == 0 it is the context's tables as its encoder writes them into a header, and the call is an encode from patches.
 *   container parts  the view decoder's sequence up to the gather on the decode slots, the part's rectangle as the view's: route 0 with a
 *                    usable index of version 1 or 2, else route 1.  MPC_VIEW_PARSE_ALL and what is trusted without it are the views',
 *                    word for word.  Behind the gather the paste kernel writes from the slot's records straight into the call's
 *                    destination records, after the slot's error words have been read.  A route-0 part the device refuses starts over
 *                    on route 1.
 *   pixel parts      uploaded unless MPC_COMPOSE_DEVICE_PIXELS says the rgb pointers are device memory; mpc_encode_tiles_device over all
 *                    their tile rows with the destination's quantiser table and the context's flavour (a fast context pursues in
 *                    float); the patch is a frame of its own and is pasted with the same kernel.
 *   parts that own no tile are skipped entirely.  routes[p]: 0 or 1 for a container part, 2 for pixels, -1 for a skipped part.
 * When every paste has finished, one records-to-container job on job slot 0 makes the container.  The context's container job slots must
 * all be idle (else MPC_ERR_ARGUMENT), and they are left idle.  Parts overlap on the decode slots as a transcode's frames do; the result
 * depends neither on the number of slots nor on the order in which parts finish.
 *   index_interval < 0: no index, and `index` may be NULL.  Otherwise the interval rules of mpc_container_index (0 = the default), and
 *   *index (mpc_free) is byte for byte mpc_container_index2(out, ..., interval, MPC_INDEX_EXPANDED), made by the entropy stage.
 * A K or block size that is not the context's is MPC_ERR_ARGUMENT, reported behind the header checks; a host-only context is
 * MPC_ERR_NO_DEVICE.  On failure nothing is returned and the context stays usable. */
#define MPC_COMPOSE_DEVICE_PIXELS 2u     /* the rgb pointers of pixel parts are device memory */
mpc_status mpc_compose_indexed(mpc_context* ctx, const uint8_t* const* bytes, const size_t* nbytes, const uint8_t* const* indexes,
                               const size_t* index_bytes, int n_sources, const mpc_part* parts, int n_parts, int width, int height,
                               unsigned flags, int index_interval, uint8_t** out, size_t* out_bytes, uint8_t** index,
                               size_t* index_out_bytes, int* routes /* [n_parts] */);

/* ---- delta: encode what changed ("Encoder: changed tiles only") ----
 * The compose's fact, used from frame to frame: a tile's records depend on that tile's pixels alone, so a container made of the
 * records kept from the last frame and fresh records of the tiles whose pixels changed is, byte for byte, mpc_encode_image of the new
 * frame.  A session keeps the last frame and its records in device memory, finds the changed tiles on the device and pursues only
 * those; every container it returns is a whole frame's, a key frame for any decoder.
 *
 * mpc_changed_tiles: host only, no context; it defines what the diff kernel computes.  Tile t = tx * tiles_y + ty (tiles of
 * block_size x block_size pixels, tiles_y = ceil(height / block_size)) is CHANGED iff any of the three bytes of any pixel (x, y) of
 * it with x < width and y < height differs between prev and cur; pixel (x, y) is the 3 bytes at base + y * stride + 3 * x, a stride
 * of 0 means 3 * width.  Bytes are compared, no tile is computed.  Only pixel bytes are read: of the last row 3 * width bytes, of the
 * bytes between a row's end and the next row none.  tiles[ceil(width / block_size) * ceil(height / block_size)] receives the changed
 * tiles in ascending order, *n their number.  MPC_ERR_ARGUMENT: a null pointer, width or height < 1, block_size outside 1 ... 8, a
 * stride that is neither 0 nor at least 3 * width.
 *
 * mpc_delta_pack_geometry: host only; the packed frame of n listed tiles with at most `rows` tile rows: *packed_rows = R = min(n, rows),
 * *packed_cols = C = ceil(n / R), *packed_stride = 24 * C bytes between pixel rows, *packed_bytes = 8 * R * stride.  Listed tile j lies at
 * tile (j / R, j % R) of it, so the tile encoder's own order tx' * R + ty' over the packed frame is j.  n == 0: all four are 0.
 * MPC_ERR_ARGUMENT: a null pointer, n < 0 or n >= 2^31, rows < 1.  The one function the pack launch and the tests share. */
mpc_status mpc_changed_tiles(const uint8_t* prev, size_t prev_stride, const uint8_t* cur, size_t cur_stride, int width, int height,
                             int block_size, int32_t* tiles, int* n);
mpc_status mpc_delta_pack_geometry(long long n, int rows, int* packed_rows, int* packed_cols, size_t* packed_stride, size_t* packed_bytes);

/* The three kernels on the caller's buffers, asynchronous on `stream`, tiles of 8 x 8 pixels.  Each: MPC_ERR_ARGUMENT, with nothing
 * enqueued, for a null pointer, width or height < 1, a row_stride that is neither 0 (= 3 * width) nor at least 3 * width;
 * MPC_ERR_NO_DEVICE for a host-only context.
 *   mpc_tile_diff_device      mpc_changed_tiles(d_kept, 0, d_rgb, row_stride, width, height, 8, ...) into d_list[tiles] / *d_count (int32),
 *                             and d_kept (height rows of 3 * width bytes, tightly packed) overwritten with the new pixels.  d_rgb follows
 *                             the frame layout rules of mpc_encode_tiles_device: any base, any stride, only pixel bytes are read; 8-byte
 *                             fetches when both bases, row_stride and 3 * width are multiples of 8, byte by byte otherwise.  The list's
 *                             order is the tiles' own, whatever the kernels' schedule.  The flags and the per-block counts live in a
 *                             scratch of the context (grown on demand, which synchronises the device): calls of one context go on one
 *                             stream, or are ordered by the caller.  d_kept and d_rgb must not overlap.
 *   mpc_pack_tiles_device     the n listed tiles of the frame, side by side, as the packed frame mpc_delta_pack_geometry(n, rows) describes, in
 *                             d_packed (8-byte aligned; packed_stride 0 = 24 * C, else a multiple of 8 and at least 24 * C, else
 *                             MPC_ERR_ARGUMENT; bytes of a row behind 24 * C are not written).  Black (0, 0, 0): the pixels of a listed tile
 *                             that lie outside the image, the R * C - n padding tiles, and a list entry outside [0, tiles), which reads
 *                             nothing.  Black is exact: YUVFromRGB(0, 0, 0) is +0.0 in all three channels, which is what the tile encoder's
 *                             zero fill gives the out-of-image pixels of a ragged tile.  n < 1 or rows < 1: MPC_ERR_ARGUMENT.
 *   mpc_scatter_records_device  records j of the packed frame (counts[j * 3 + ch], choices[(j * 3 + ch) * K + i], K the context's) copied to
 *                             tile d_list[j] of the whole-frame records of `tiles` tiles: a plain copy (the tile encoder zeroes the entries
 *                             beyond a count).  A list entry outside [0, tiles) is skipped and sets the context's crop error word
 *                             (mpc_crop_records_check reads and clears it).  The entries must be distinct.  n < 1 or tiles < 1:
 *                             MPC_ERR_ARGUMENT. */
mpc_status mpc_tile_diff_device(mpc_context* ctx, uint8_t* d_kept, const uint8_t* d_rgb, int width, int height, size_t row_stride,
                                int32_t* d_list, int32_t* d_count, void* stream);
mpc_status mpc_pack_tiles_device(mpc_context* ctx, const uint8_t* d_rgb, int width, int height, size_t row_stride, const int32_t* d_list,
                                 int n, int rows, uint8_t* d_packed, size_t packed_stride, void* stream);
mpc_status mpc_scatter_records_device(mpc_context* ctx, const uint16_t* d_packed_counts, const mpc_basis_choice* d_packed_choices,
                                      const int32_t* d_list, int n, uint16_t* d_counts, mpc_basis_choice* d_choices, int tiles, void* stream);

/* A session: frames of width x height, one after the other, through one context.  It owns, on the context's device: the last frame
 * (tightly packed), the whole frame's records, the list, and -- grow-only, sized by the largest call so far -- a host frame's copy and
 * the packed frame with its records.  It must be destroyed before its context.  mpc_delta_create: MPC_ERR_ARGUMENT for a null pointer
 * or width or height < 1, MPC_ERR_NO_DEVICE for a host-only context.
 *
 * mpc_delta_encode is synchronous, like mpc_encode_image.  rgb: the frame, host memory unless MPC_DELTA_DEVICE_PIXELS; row_stride 0 =
 * 3 * width; the frame layout rules of mpc_encode_tiles_device.  quant: 3K doubles or NULL = the context's tables as they are now.
 * THE CONTRACT: *bytes (mpc_free) is byte for byte what mpc_encode_image_device returns for this frame with this quantiser table and
 * the context's flavour, whatever the history of the session.  index_interval < 0: no index, `index` may be NULL; otherwise
 * mpc_container_index's interval rules (0 = the default) and *index (mpc_free) is byte for byte mpc_container_index2(*bytes, ...,
 * interval, MPC_INDEX_EXPANDED), made by the entropy stage.
 * A call is a KEY FRAME when it is the session's first, when MPC_DELTA_KEY is set, when any of the 3K doubles of the quantiser table
 * differs from the previous successful call's, when the context's fast flag does, or when the previous call failed behind its checks.
 * A key frame is pursued whole, straight into the record store (with MPC_DELTA_PACK_ALWAYS through list -> pack -> encode -> scatter
 * like any other, with every tile listed); info->changed = info->tiles, info->key = 1.
 * Any other call: the frame is uploaded unless it is device memory; the diff kernel lists the changed tiles and brings the kept copy
 * up to date; their number n is read back (the call waits for it); with n > 0 the pack kernel makes the packed frame of
 * MPC_DELTA_PACK_ROWS tile rows at most, mpc_encode_tiles_device pursues it with the call's table, and the scatter kernel puts its
 * records into the store; with n == 0 no pursuit is launched (mpc_kernel_timing_read counts 0 launches).  Then, key frame or not, one
 * records-to-container job on job slot 0 makes the container from the store, exactly as mpc_compose_indexed finishes.
 * Refused with nothing enqueued and the session unchanged (the next call is still a delta): MPC_ERR_ARGUMENT for a null pointer
 * (`index` and `index_bytes` only with index_interval >= 0), an unknown flag, an interval outside the rules, row_stride != 0 &&
 * row_stride < 3 * width, a container job slot that is not idle; MPC_ERR_NO_DEVICE for a host-only context.  A failure behind these
 * checks returns nothing, leaves the context usable and the slots idle, and invalidates the session: its next call is a key frame.
 *
 * mpc_delta_changed: the last successful call's list, ascending (a key frame's: every tile); *n its length, also when `capacity` is
 * too small for it: then MPC_ERR_ARGUMENT and nothing is copied, except that capacity == 0 only asks for *n. */
typedef struct mpc_delta mpc_delta;
typedef struct mpc_delta_info { int tiles, changed, key; } mpc_delta_info;
#define MPC_DELTA_KEY            1u   /* pursue every tile whatever the diff says */
#define MPC_DELTA_DEVICE_PIXELS  2u   /* rgb is device memory */
#define MPC_DELTA_PACK_ALWAYS    4u   /* tests: a key frame too goes list -> pack -> encode -> scatter */
#define MPC_DELTA_PACK_ROWS      64   /* tile rows of the packed frame; it only shapes the tile encoder's queue order */
mpc_status mpc_delta_create(mpc_context* ctx, int width, int height, mpc_delta** out);
void       mpc_delta_destroy(mpc_delta* d);
mpc_status mpc_delta_encode(mpc_delta* d, const uint8_t* rgb, size_t row_stride, const double* quant, unsigned flags, int index_interval,
                            uint8_t** bytes, size_t* nbytes, uint8_t** index, size_t* index_bytes, mpc_delta_info* info);
mpc_status mpc_delta_changed(const mpc_delta* d, int32_t* tiles, int capacity, int* n);   /* the last call's list */

/* ---- delta with a change tolerance ("Encoder: a change tolerance") ----
 * A camera, a dithered render or a lossy hop changes a few low bits in every tile of every frame; with a tolerance the caller says that
 * differences this small are not a change.  THE DEFINITION, host, exact, integer: sse(t) = the sum of (cur - kept)^2 over the three
 * bytes of every pixel of tile t that lies inside the image (mpc_changed_tiles's tiles, order and reads; at most 64 * 3 * 255^2 =
 * 12 484 800, exact in 32 bits in any order).  Tile t is CHANGED iff sse(t) > tolerance and HELD iff 0 < sse(t) <= tolerance.  After
 * the diff the kept copy holds cur's pixels in every changed tile and its old pixels, whole, in every other.  So a session keeps the
 * COMPOSITE C_n: C_n = frame n for a key frame; else, tile by tile, frame n where the tile is changed and C_(n-1) where it is not.  A
 * held tile is compared with the pixels last SENT, not with the previous frame: a slow drift adds up until it crosses the tolerance
 * and is sent then, and at every call every tile of C_n is within `tolerance` of frame n's.  tolerance 0 is the rule above exactly
 * (sse > 0: some byte differs); 12 484 800 or more holds everything but key frames, which is allowed.
 *
 * mpc_changed_tiles_tolerance: mpc_changed_tiles's arguments, rules and refusals, plus the tolerance and sse: NULL or one value per
 * tile, every tile's.  prev is not written: the composite is cur in the listed tiles, prev elsewhere.
 * mpc_tile_diff_tolerance_device: mpc_tile_diff_device's layout rules, refusals, scratch and stream contract (asynchronous on `stream`,
 * nothing on the null stream), with d_kept brought up to the composite; d_sse: NULL or tiles values in device memory.
 *
 * THE SESSION.  mpc_delta_set_tolerance: session state, 0 at first, read by the next call; it makes no key frame and leaves the sent
 * map valid.  MPC_ERR_ARGUMENT for a null session.  mpc_delta_tolerance reads it back (0 for a null session).  At tolerance 0 a call
 * enqueues exactly what it did before there was a tolerance.  Key-frame rules are unchanged and a key frame copies the frame whole.
 * THE CONTRACTS, restated with the composite:
 *   mpc_delta_encode                  every container is byte for byte mpc_encode_image_device of C_n, its index that container's
 *   mpc_delta_encode_patch[_indexed]  a receiver that applied every patch holds, after call n, the decode of C_n's container
 *   mpc_delta_encode_patch_budget     the invariant of "rate" with "the current frame's full records" read as C_n's; the tiles that
 *                                     must be sent are the tolerant diff's list
 *   mpc_delta_changed                 the tolerant list
 * The emphasis map does not scale the tolerance.
 * mpc_delta_held: the last successful call's held tiles and the sum of their sse; both 0 for a key frame and at tolerance 0.
 * held_sse / (3 * width * height) is the mean squared error of C_n against frame n: its PSNR without a decode.
 * mpc_delta_frame_device: C_n, the session's own buffer, height rows of 3 * width bytes, valid until the next call;
 * mpc_delta_frame: its copy to the host (row_stride 0 = 3 * width).  Both: MPC_ERR_ARGUMENT for a null pointer, a row_stride below
 * 3 * width, or a session without a frame (no successful call yet, or the last one failed behind its checks).
 * A refused encode call leaves the tolerance, the composite and the held totals as they were. */
mpc_status mpc_changed_tiles_tolerance(const uint8_t* prev, size_t prev_stride, const uint8_t* cur, size_t cur_stride, int width, int height,
                                       int block_size, uint32_t tolerance, int32_t* tiles, int* n, uint32_t* sse /* NULL or [tiles] */);
mpc_status mpc_tile_diff_tolerance_device(mpc_context* ctx, uint8_t* d_kept, const uint8_t* d_rgb, int width, int height, size_t row_stride,
                                          uint32_t tolerance, int32_t* d_list, int32_t* d_count, uint32_t* d_sse /* NULL or [tiles] */,
                                          void* stream);
mpc_status mpc_delta_set_tolerance(mpc_delta* d, uint32_t tolerance);
uint32_t   mpc_delta_tolerance(const mpc_delta* d);
mpc_status mpc_delta_held(const mpc_delta* d, int* held, uint64_t* held_sse);
mpc_status mpc_delta_frame(mpc_delta* d, uint8_t* rgb, size_t row_stride);
mpc_status mpc_delta_frame_device(mpc_delta* d, uint8_t** d_rgb);

/* ---- patch: send only the changed tiles, apply them on the device ("Delta stream") ----
 * The packed frame of a delta call's listed tiles is an ordinary frame, so its container is an ordinary container.  A PATCH is the
 * ascending tile list plus that container: what a receiver that holds the previous frame needs, at a few per cent of the bytes.
 *
 * THE FORMAT, version 1, little endian:
 *    0 "MPCP" | 4 u16 version = 1 | 6 u16 flags: bit 0 = key, every other bit 0 | 8 u32 width | 12 u32 height | 16 u32 sequence |
 *   20 u32 n (tiles listed) | 24 u32 list_bytes | 28 u32 0 | 32 u64 container_bytes | 40 the list, then the container
 * and the patch is exactly 40 + list_bytes + container_bytes long.  The list holds the gaps of the ascending tile list, g0 = t0,
 * gj = tj - t(j-1) - 1, each as LEB128: 7 bits a byte, low group first, at most 5 bytes, value below 2^31; a multi-byte value whose
 * last byte is 0x00 is refused.  Ascending order and distinctness hold by construction; exactly n values fill exactly list_bytes; the
 * last tile is below tiles = ceil(width / 8) * ceil(height / 8) (tile t = tx * tiles_y + ty, as everywhere).  Three forms:
 *   key    flag set, n = tiles, list_bytes = 0; the container is the whole frame's (width x height)
 *   empty  no flag, n = 0, list_bytes = 0, container_bytes = 0: 40 bytes
 *   tile   no flag, 0 < n < tiles; the container's header says 8C x 8R pixels with (R, C) = mpc_delta_pack_geometry(n,
 *          MPC_DELTA_PACK_ROWS) -- the 64 is part of format version 1 -- and listed tile j is tile (j / R, j % R) of it
 * There is no patch with n == tiles and no key flag: the sender writes a key patch instead.
 * VERSION 2 is version 1 with one word given a meaning and one section appended ("patch index", further down): version = 2, the word
 * at 28 = index_bytes (> 0), and index_bytes of the container's seek index behind the container.  Everything in this section reads a
 * version-2 patch as it reads the patch without its index; only the receiver's decode (step 4) takes another route to the same pixels.
 *
 * Host only, no context:
 *   mpc_patch_make   the only writer: *bytes (mpc_free).  key != 0: n must be the frame's tile count, `tiles` is not read; else n == 0
 *                    with container_bytes == 0, or 0 < n < tiles with tiles[n] ascending, distinct and inside the frame.  The container's
 *                    bytes are copied as they are (mpc_patch_info is what checks them), so a whole-frame container from anywhere
 *                    becomes a key patch.  MPC_ERR_ARGUMENT for anything else.
 *   mpc_patch_info   validates the patch whole -- header, form, list, length, and the container's own header through
 *                    mpc_container_info and its size against the form -- and reports it; container_offset is from `bytes`.
 *   mpc_patch_tiles  the list (a key patch's: every tile); *n its length, also when `capacity` is too small: then MPC_ERR_ARGUMENT and
 *                    nothing is copied, except that capacity == 0 only asks for *n.
 * A refused patch is MPC_ERR_BITSTREAM, a null pointer or bad geometry MPC_ERR_ARGUMENT; nothing in a header is trusted, nothing is
 * read outside [bytes, bytes + nbytes), and no more is allocated than the patch is long.
 *
 * THE SENDER, mpc_delta_encode_patch: mpc_delta_encode's flags, refusals and stages up to the records (frame on the device, list,
 * pursuit and scatter), so a session's store advances identically whichever of the two is called, in any mix.  A call is a key
 * frame by mpc_delta_encode's rule, and sent as a key patch also when the diff lists every tile (info->key = 1 then too).
 *   key patch    the container from the store: byte for byte mpc_encode_image_device of the frame
 *   tile patch   the same container job, on job slot 0, run on the packed frame's counts and records at 8C x 8R: byte for byte
 *                mpc_encode_image_device of the packed frame mpc_pack_tiles_device makes of the list
 *   empty patch  no pursuit launch and no container job
 * `sequence` is the number of successful calls of either kind the session had before this one.  *patch: mpc_free.
 *
 * mpc_unpack_tiles_device: mpc_pack_tiles_device's inverse on the caller's buffers, asynchronous on `stream`.  The pixel bytes of listed
 * tile j, at tile (j / R, j % R) of the packed frame mpc_delta_pack_geometry(n, rows) describes (d_packed 8-byte aligned; packed_stride
 * 0 = 24 * C, else a multiple of 8 and at least 24 * C), go to tile d_list[j] of the frame at d_rgb (row_stride 0 = 3 * width; any
 * base, any stride).  Only bytes inside the image are written: none at or behind 3 * width of a row, no row at or below height,
 * nothing for the R * C - n padding tiles, nothing of any other tile.  8-byte stores where d_rgb and row_stride are multiples of 8
 * and the chunk lies whole inside its row, byte by byte otherwise.  A list entry outside [0, tiles) writes nothing and sets the
 * context's crop error word (mpc_crop_records_check reads and clears it).  The argument rules of the three kernels above.
 *
 * THE RECEIVER: a session that owns, on the context's device, the current frame (tightly packed, black until the first key patch),
 * a grow-only staging area for decoded pixels, the list and a stream.  It keeps no records.  Destroy it before its context.
 * mpc_patch_apply is synchronous:
 *   1. mpc_patch_info's checks on the host; width and height must be the session's (else MPC_ERR_ARGUMENT)
 *   2. a key patch sets expected = sequence + 1; any other patch needs a session that has had a key patch and sequence == expected,
 *      else MPC_ERR_ARGUMENT with both numbers in mpc_last_error
 *   3. the container's block size and K must be the context's (MPC_ERR_ARGUMENT)
 *   4. key patch: mpc_decode_image_device into staging, then one device copy to the frame.  Tile patch: the same decode of the packed
 *      frame into staging, the list uploaded, the unpack kernel.  Empty patch: only the sequence advances.
 * ATOMIC: a refusal -- a bad patch, a container the decoder refuses (its status and text), one of the wrong size, a wrong sequence,
 * a wrong block size or K -- leaves the frame, the list and the expected sequence exactly as they were; nothing reaches the frame
 * before every check has passed and the container is decoded whole.  (A device failure behind that, MPC_ERR_HIP, leaves a session
 * that wants a key patch.)  The decode takes the context's flavour, as mpc_decode_image does.
 *   mpc_patch_frame_device  the kept frame, height rows of 3 * width bytes, valid until the next apply
 *   mpc_patch_read          its copy to the host (row_stride 0 = 3 * width)
 *   mpc_patch_changed       the last successful apply's list, with mpc_delta_changed's rules */
struct mpc_patch_info {
    int width, height;
    uint32_t sequence;
    int key;
    int n, tiles;                              /* tiles listed (a key patch: all), tiles of the frame */
    size_t container_offset, container_bytes;
};
mpc_status mpc_patch_make(int width, int height, uint32_t sequence, int key, const int32_t* tiles, int n, const uint8_t* container,
                          size_t container_bytes, uint8_t** bytes, size_t* nbytes);
mpc_status mpc_patch_info(const uint8_t* bytes, size_t nbytes, struct mpc_patch_info* info);
mpc_status mpc_patch_tiles(const uint8_t* bytes, size_t nbytes, int32_t* tiles, int capacity, int* n);
mpc_status mpc_delta_encode_patch(mpc_delta* d, const uint8_t* rgb, size_t row_stride, const double* quant, unsigned flags, uint8_t** patch,
                                  size_t* patch_bytes, mpc_delta_info* info);
mpc_status mpc_unpack_tiles_device(mpc_context* ctx, const uint8_t* d_packed, size_t packed_stride, const int32_t* d_list, int n, int rows,
                                   uint8_t* d_rgb, int width, int height, size_t row_stride, void* stream);
typedef struct mpc_patch_decoder mpc_patch_decoder;
mpc_status mpc_patch_decoder_create(mpc_context* ctx, int width, int height, mpc_patch_decoder** out);
void       mpc_patch_decoder_destroy(mpc_patch_decoder* p);
mpc_status mpc_patch_apply(mpc_patch_decoder* p, const uint8_t* patch, size_t nbytes, struct mpc_patch_info* info);
mpc_status mpc_patch_frame_device(mpc_patch_decoder* p, uint8_t** d_rgb);
mpc_status mpc_patch_read(mpc_patch_decoder* p, uint8_t* rgb, size_t row_stride);
mpc_status mpc_patch_changed(const mpc_patch_decoder* p, int32_t* tiles, int capacity, int* n);

/* ---- budget: encode to a byte budget ("Encoder: a byte budget") ----
 * The container is layered by pursuit step, every tile-channel has its own length and nothing reads a record beyond its count: cutting
 * a tile to its first n steps is a change of three counts, and the result is a container every decoder reads unchanged.  The search
 * below picks a depth per tile, spending the bytes where they lower the error most, from one pursuit and a handful of container jobs.
 * Frames of 8 x 8 tiles, T tiles, K the context's; whole-frame records (tile t = tx * tiles_y + ty, counts[t * 3 + ch],
 * choices[(t * 3 + ch) * K + i]).  Host and device agree bit for bit on everything defined here.
 *
 * DEPTH PROFILE  P[t][n], n = 0 ... K, u32 at profile[t * (K + 1) + n]: the value mpc_distortion_device's d_tile_sse[t] has for the same
 * records with every count replaced by min(count, n) -- the decoder's flavour (the fast flag), the header's u16 quantiser steps, the
 * integer dr^2 + dg^2 + db^2 over the pixels inside the frame; n = 0 is the all-black tile.  Defined for PREFIX-CONSISTENT records: the
 * row of record i lies in the dynamic dictionary built from choices 0 ... i - 1, which holds for every encoder's records.  A record that
 * is not (a forward reference, a row outside its dictionary) and a count above K set the context's crop error word
 * (mpc_crop_records_check: MPC_ERR_BITSTREAM "Invalid bitstream"); that tile's profile is then unspecified, and no address comes from it.
 * RATE WEIGHTS  W[ch][i], u32 in 1/256 bit at weights[ch * K + i], from a seek index (either version) of the frame's FULL container:
 * with a = 1 + 2K * ch + 2i, bits = end_bit(a + 1) - wrapper_bit(a) and n = expect(a): W = clamp((256 * bits + n / 2) / n, 256, 2^20),
 * and 256 when n = 0 -- the average cost of a record of that channel and step, wrappers and tables included.
 * RATE OF A DEPTH  R[t][n] = sum over ch and i < min(n, counts[t * 3 + ch]) of W[ch][i], below 2^27.
 * MULTIPLIERS  L[0] = 0, L[j] = (8 + (j - 1) % 8) << ((j - 1) / 8) for j = 1 ... 255 (MPC_BUDGET_LAMBDAS entries), u64.
 * ALLOCATION AT j  J(t, n) = P[t][n] * 65536 + L[j] * R[t][n] in u64 (P < 2^24, L < 2^35: no overflow); depth[t] = the smallest n that
 * minimises J; the cut counts are min(count, depth[t]); totals[0] = sum of P[t][depth[t]], totals[1] = sum of R[t][depth[t]], totals[2] =
 * the records kept.  A count above K is used as K.  At j = 255 every depth is 0 (for a profile that repeats above a tile's largest count).
 *
 * mpc_budget_lambda: *lambda = L[j]; MPC_ERR_ARGUMENT outside 0 ... 255.
 * mpc_budget_weights: weights[3K], K the index's.  MPC_ERR_BITSTREAM for what mpc_index_info refuses, MPC_ERR_ARGUMENT for a serial-only
 * index (it holds no stream sizes) and for a null pointer.
 * mpc_budget_allocate: the allocation on the host; it defines what the kernel computes.  depth[tiles] and out_counts[3 * tiles]: each NULL or
 * room for that; totals[3].  MPC_ERR_ARGUMENT: a null pointer, tiles < 0, K outside 1 ... 32, j outside 0 ... 255.
 * The three are host only, need no context and are safe on several threads.
 *
 * mpc_depth_profile_device: the profile of the records against the frame they came from (d_rgb: 3 * width bytes a row, tightly packed),
 * all in device memory, into d_profile[tiles * (K + 1)].  quant as for mpc_distortion_device.  Asynchronous on `stream`.
 * mpc_budget_allocate_device: the allocation of `tiles` tiles (K the context's) with weights[3K] in HOST memory (they travel in the
 * kernel's arguments): d_depth[tiles] (u8), d_out_counts[3 * tiles], d_totals[3] (u64; zeroed on `stream` first).  Asynchronous.
 * Both: MPC_ERR_ARGUMENT with nothing enqueued for a null pointer or a geometry outside mpc_rate_distortion's, MPC_ERR_NO_DEVICE for a
 * host-only context.
 *
 * mpc_encode_image_budget[_device]: a container of at most `budget` bytes of the frame (host: 3 * width bytes a row; _device: device
 * memory, tightly packed).  Synchronous.
 *   1. the whole frame is pursued once; the records stay on the device
 *   2. the full container F with its seek index is made on job slot 0, the way mpc_delta_encode finishes
 *   3. |F| <= budget: F is returned, byte for byte mpc_encode_image; lambda_index = -1, probes = 0, every depth K
 *   4. else the weights are taken from F's index and the profile is made, once
 *   5. size(j) is the container of the cut counts at j: the same job on the same records with the cut counts array
 *   6. size(255) > budget: MPC_ERR_ARGUMENT, the budget and size(255) in the text
 *   7. bisection with lo = -1 (infeasible) and hi = 255 (feasible), mid = (lo + hi) / 2 rounded down (127 first): size(mid) <= budget
 *      moves hi, else lo moves, until hi = lo + 1
 *   8. hi's container is returned, kept from its probe: nothing is coded twice
 * At most nine probes, size(255) among them.  The size need not be monotone in j: what the result promises is the two invariants, lo
 * infeasible and hi feasible.  quant: 3K doubles or NULL = the context's tables.  index_interval < 0: no index, `index` may be NULL;
 * otherwise mpc_container_index's interval rules (0 = the default) and *index (mpc_free) is byte for byte mpc_container_index2(*bytes,
 * ..., interval, MPC_INDEX_EXPANDED) of the returned container.  depth: NULL, or host room for the returned container's depth per tile.
 * info: lambda_index, probes, full_bytes = |F|, sse and records of the returned container (what mpc_decode_image of it differs from the
 * frame by, exactly), full_sse and full_records of F.
 * Refused with nothing enqueued: MPC_ERR_ARGUMENT for a null pointer (`index` and `index_bytes` only with index_interval >= 0), a geometry
 * outside mpc_rate_distortion's, budget = 0, an interval outside the rules, a container job slot that is not idle; MPC_ERR_NO_DEVICE for a
 * host-only context.  On failure nothing is returned, the slots are idle and the context is usable.  The call leaves the context's quant
 * tables, fast flag and workgroup limit as it found them. */
#define MPC_BUDGET_LAMBDAS 256
typedef struct mpc_budget_info {
    int lambda_index, probes;
    size_t full_bytes;
    unsigned long long sse, full_sse, records, full_records;
} mpc_budget_info;
int mpc_budget_lambda(int j, uint64_t* lambda);
mpc_status mpc_budget_weights(const uint8_t* index, size_t index_bytes, uint32_t* weights /* [3K] */);
mpc_status mpc_budget_allocate(const uint32_t* profile, const uint16_t* counts, long long tiles, int K, const uint32_t* weights, int j,
                               uint8_t* depth, uint16_t* out_counts, uint64_t* totals);
mpc_status mpc_depth_profile_device(mpc_context* ctx, const uint16_t* d_counts, const mpc_basis_choice* d_choices, const double* quant,
                                    const uint8_t* d_rgb, int width, int height, uint32_t* d_profile, void* stream);
mpc_status mpc_budget_allocate_device(mpc_context* ctx, const uint32_t* d_profile, const uint16_t* d_counts, long long tiles,
                                      const uint32_t* weights, int j, uint8_t* d_depth, uint16_t* d_out_counts, unsigned long long* d_totals,
                                      void* stream);
mpc_status mpc_encode_image_budget(mpc_context* ctx, const uint8_t* rgb, int width, int height, const double* quant, size_t budget,
                                   int index_interval, uint8_t** bytes, size_t* nbytes, uint8_t** index, size_t* index_bytes, uint8_t* depth,
                                   mpc_budget_info* info);
mpc_status mpc_encode_image_budget_device(mpc_context* ctx, const uint8_t* d_rgb, int width, int height, const double* quant, size_t budget,
                                          int index_interval, uint8_t** bytes, size_t* nbytes, uint8_t** index, size_t* index_bytes,
                                          uint8_t* depth, mpc_budget_info* info);

/* ---- quality: encode to a target quality ("Encoder: a target quality") ----
 * The budget section turned round: not "the best frame in N bytes" but "the smallest container whose decode is at least this good".
 * Distortion, unlike a size, needs no container to be known: the squared error of a cut is the sum of the depth profile at the chosen
 * depths, exactly.  So the search makes no probe: one kernel evaluates the allocation at all 256 multipliers, the host picks one from
 * 256 x 3 integers, and one allocation and one container job finish the call.  Everything named here (P, W, R, L[j], J, the allocation
 * at j and its totals) is the budget section's.  Host and device agree bit for bit.
 *
 * SWEEP  S[j][k], j = 0 ... 255, k = 0 ... 2, u64 at totals[3 * j + k]: exactly the totals[k] that mpc_budget_allocate returns at
 * multiplier j for the same profile, counts and weights -- S[j][0] the distortion, S[j][1] the rate in 1/256 bit, S[j][2] the records
 * kept.  A count above K is used as K; the smallest n wins on ties.  Weights as mpc_budget_weights makes them (256 ... 2^20).
 * L[j] rises strictly with j, so S[j][0] never falls and S[j][1] never rises along the ladder, also for a profile that is not monotone
 * in depth (for one tile, add the optimality inequalities of the minimisers at two multipliers).  S[0][0] is the sum of every tile's
 * least profile entry: the best quality cutting can reach; it can lie below the full container's squared error.
 * PICK at max_sse: the largest j with S[j][0] <= max_sse, -1 if there is none.
 *
 * mpc_budget_sweep: the sweep on the host; it defines what the kernel computes.  totals[768].  It refuses what mpc_budget_allocate
 * refuses: MPC_ERR_ARGUMENT for a null pointer, tiles < 0, K outside 1 ... 32.
 * mpc_quality_pick: the pick among totals[768]; -1 also for totals == NULL.
 * mpc_sse_for_psnr: *max_sse = the largest integer s in 0 ... 195075 * 64 * tiles (tiles of 8 x 8 of the geometry) whose PSNR at
 * width x height -- mpc_psnr's formula, 20 log10(765) - 10 log10(s / (width * height)) -- is >= psnr: found by a binary search on
 * that very function, so it agrees with mpc_psnr and mpc_rate_distortion to the bit.  s = 0 has PSNR +inf, so every target has an
 * answer: +inf gives 0.  MPC_ERR_ARGUMENT: NaN, -inf, a null pointer, a geometry outside mpc_rate_distortion's.
 * The three are host only, need no context and are safe on several threads.
 *
 * mpc_budget_sweep_device: the sweep of `tiles` tiles (K the context's) with weights[3K] in HOST memory (they travel in the kernel's
 * arguments) into d_totals[768] (u64; zeroed on `stream` first): one launch for all 256 multipliers.  Asynchronous on `stream`.
 * mpc_budget_allocate_device's refusals, with nothing enqueued: MPC_ERR_ARGUMENT for a null pointer, tiles outside
 * mpc_rate_distortion's geometry, a stream that is being captured; MPC_ERR_NO_DEVICE for a host-only context.
 *
 * mpc_encode_image_quality[_device]: the frame (host: 3 * width bytes a row; _device: device memory, tightly packed) as the container
 * of the allocation at the largest multiplier whose squared error is at most max_sse.  Synchronous.
 *   1. the whole frame is pursued once; the records stay on the device
 *   2. the full container F with its seek index is made on job slot 0, as in the budget encode
 *   3. the weights are taken from F's index and the depth profile is made, once
 *   4. the sweep: one launch; the 768 totals go to the host
 *   5. j = the pick at max_sse
 *   6. j = -1: MPC_ERR_ARGUMENT, max_sse and S[0][0] in the text
 *   7. the allocation kernel at j
 *   8. one container job on the same records with the cut counts, and with it the index if asked for
 *   9. that container is returned
 * Two container jobs, no per-multiplier launch, and no early return of F: a target looser than F's own squared error still yields the
 * cut at the pick, which keeps no more records than F and as a rule far fewer.  What the result promises: info->sse <= max_sse, and j is the largest multiplier of the
 * ladder for which that holds.  The returned length is whatever the entropy coder makes of that allocation: the rate model is an
 * average per stream, so the byte count is NOT promised minimal, nor monotone in max_sse.  max_sse = 0 is a valid request: a lossless
 * result, or the refusal of step 6.
 * quant, index_interval, *index, depth: as for mpc_encode_image_budget (*index byte for byte mpc_container_index2(*bytes, ..., interval,
 * MPC_INDEX_EXPANDED) of the returned container).  info: lambda_index = j; full_bytes = |F|; sse = S[j][0], what mpc_decode_image of the
 * result differs from the frame by, exactly; full_sse that of F; min_sse = S[0][0]; records = S[j][2] and full_records those of F;
 * model_bits_256 = S[j][1].
 * Refusals and side effects are the budget encode's: refused with nothing enqueued, MPC_ERR_ARGUMENT for a null pointer (`index` and
 * `index_bytes` only with index_interval >= 0), a geometry outside mpc_rate_distortion's, an interval outside the rules, a container
 * job slot that is not idle; MPC_ERR_NO_DEVICE for a host-only context.  On failure nothing is returned, the slots are idle and the
 * context is usable.  The call leaves the context's quant tables, fast flag and workgroup limit as it found them. */
typedef struct mpc_quality_info {
    int lambda_index;
    size_t full_bytes;
    unsigned long long sse, full_sse, min_sse, records, full_records, model_bits_256;
} mpc_quality_info;
mpc_status mpc_budget_sweep(const uint32_t* profile, const uint16_t* counts, long long tiles, int K, const uint32_t* weights,
                            uint64_t* totals /* [256 * 3] */);
int mpc_quality_pick(const uint64_t* totals /* [256 * 3] */, uint64_t max_sse);
mpc_status mpc_sse_for_psnr(double psnr, int width, int height, uint64_t* max_sse);
mpc_status mpc_budget_sweep_device(mpc_context* ctx, const uint32_t* d_profile, const uint16_t* d_counts, long long tiles,
                                   const uint32_t* weights /* host, [3K] */, unsigned long long* d_totals /* [768] */, void* stream);
mpc_status mpc_encode_image_quality(mpc_context* ctx, const uint8_t* rgb, int width, int height, const double* quant,
                                    unsigned long long max_sse, int index_interval, uint8_t** bytes, size_t* nbytes, uint8_t** index,
                                    size_t* index_bytes, uint8_t* depth, mpc_quality_info* info);
mpc_status mpc_encode_image_quality_device(mpc_context* ctx, const uint8_t* d_rgb, int width, int height, const double* quant,
                                           unsigned long long max_sse, int index_interval, uint8_t** bytes, size_t* nbytes,
                                           uint8_t** index, size_t* index_bytes, uint8_t* depth, mpc_quality_info* info);

/* ---- rate: a delta stream to a byte budget ("Delta stream to a byte budget") ----
 * A patch is as large as the scene makes it; a link has a byte rate.  A sender that cuts patches to a budget must know what the
 * receiver holds of each tile, and may refine a thin tile later.  These are the pieces of that sender: the state (a depth per tile),
 * which tiles a call may send, the allocation when a tile has a floor, and the gather that makes a packed frame's records from the
 * whole frame's.  8 x 8 tiles, T tiles a frame, K the context's, tile t = tx * tiles_y + ty as everywhere.  Host and device agree bit
 * for bit on everything defined here.
 *
 * SENT DEPTH  sent[t], u8, 0 ... K: the receiver's tile t is the decode of tile t's records with every count cut to min(count, sent[t]).
 * full(t) = max over ch of min(counts[t * 3 + ch], K).  Tile t is OWED iff sent[t] < full(t).
 * CANDIDATES of a call: the changed tiles plus the owed tiles, ascending.  A changed tile MUST be sent, its floor is 0.  An owed,
 * unchanged tile MAY be sent, its floor is sent[t]; not sending it costs no bytes and leaves it as it is.  Sending always sends a tile's
 * records from step 0.
 * ALLOCATION WITH A FLOOR at multiplier j, per candidate i with profile P[i][0 ... K], three counts, floor[i] (above K: used as K) and
 * must[i]; W, L[j] and R[i][n] as in the budget section.  Allowed depths: every n in 0 ... K when must[i], else floor[i] and every n above
 * it.  R'(i, n) = R[i][n], except R'(i, floor[i]) = 0 for a candidate with must[i] == 0.  J = 65536 * P[i][n] + L[j] * R'(i, n) in u64;
 * depth[i] = the smallest allowed n that minimises J; send[i] = must[i] || depth[i] > floor[i]; out_counts = min(count, depth[i]);
 * totals[0] = sum of P at the chosen depths, [1] = sum of R', [2] = the records kept in the candidates that are sent, [3] = the
 * candidates sent.  With every candidate must and every floor 0 it is mpc_budget_allocate bit for bit (depth, out_counts, totals[0 ... 2]).
 *
 * Host only, no context, safe on several threads; they define what the kernels compute:
 *   mpc_owed_tiles             sent[tiles], counts[3 * tiles], changed[n_changed] (ascending, distinct, inside the frame) -> candidates
 *                              (room for `tiles`), *n their number, and PER TILE must[t] = 1 iff t is changed, floor[t] = 0 for a
 *                              changed tile, else sent[t].  candidates, floor, must: each NULL or room for `tiles`.
 *   mpc_budget_allocate_floor  floor, must: NULL = all 0, all 1.  depth[n], out_counts[3 * n], send[n]: each NULL or room; totals[4].
 * MPC_ERR_ARGUMENT: a null pointer, tiles or n < 0, K outside 1 ... 32, j outside 0 ... 255, a changed list that breaks its rules.
 *
 * On the caller's buffers, asynchronous on `stream`; MPC_ERR_ARGUMENT with nothing enqueued for a null pointer (unless named optional)
 * or a size below 1, MPC_ERR_NO_DEVICE for a host-only context:
 *   mpc_owed_tiles_device      d_flags[tiles] (u8) holds, on entry, != 0 for a changed tile (the diff's flag array); the kernel ORs "owed"
 *                              into it (bit 1), writes d_floor[tiles] and d_must[tiles] as mpc_owed_tiles defines them, and the
 *                              flags -> list kernels of mpc_tile_diff_device make d_list[tiles] / *d_count (int32): the candidates in
 *                              the tiles' own order, whatever the schedule.  A count above K is used as K.  The per-block counts live
 *                              in the context's diff scratch: mpc_tile_diff_device's rule for streams.
 *   mpc_gather_records_device  mpc_scatter_records_device turned round, with a cut.  Whole-frame records of `tiles` tiles, a list
 *                              d_list[m], optionally d_idx[n] (entries in [0, m); NULL: the identity, n <= m) and d_depth[m] (NULL:
 *                              uncut) -> the records of the packed frame mpc_delta_pack_geometry(n, rows) describes: packed tile j < n
 *                              takes, with c = idx[j], the records of tile d_list[c] with the counts min(count, K, d_depth[c]); every
 *                              entry at or above that count is written as 0; every padding tile (n <= j < R * C) has counts 0 and
 *                              entries 0.  d_packed_counts[3 * R * C], d_packed_choices[3 * R * C * K]: any alignment; 16-byte pieces
 *                              where K is a multiple of 4 and both record bases are 16-byte aligned, word by word otherwise.  An
 *                              entry of d_idx outside [0, m) or of d_list outside [0, tiles) makes its packed tile all 0 and sets the
 *                              context's crop error word (mpc_crop_records_check reads and clears it); no address comes from it.
 *   mpc_budget_allocate_floor_device  the allocation of n candidates with weights[3K] in HOST memory; d_floor, d_must: each optional as
 *                              on the host; d_depth[n], d_send[n] (u8), d_out_counts[3 * n], d_totals[4] (u64; zeroed on `stream` first). */
mpc_status mpc_owed_tiles(const uint8_t* sent, const uint16_t* counts, long long tiles, int K, const int32_t* changed, int n_changed,
                          int32_t* candidates, uint8_t* floor, uint8_t* must, int* n);
mpc_status mpc_budget_allocate_floor(const uint32_t* profile, const uint16_t* counts, const uint8_t* floor, const uint8_t* must, long long n,
                                     int K, const uint32_t* weights, int j, uint8_t* depth, uint16_t* out_counts, uint8_t* send,
                                     uint64_t* totals /* [4] */);
mpc_status mpc_owed_tiles_device(mpc_context* ctx, const uint8_t* d_sent, const uint16_t* d_counts, long long tiles, uint8_t* d_flags,
                                 uint8_t* d_floor, uint8_t* d_must, int32_t* d_list, int32_t* d_count, void* stream);
mpc_status mpc_gather_records_device(mpc_context* ctx, const uint16_t* d_counts, const mpc_basis_choice* d_choices, int tiles,
                                     const int32_t* d_list, int m, const int32_t* d_idx, const uint8_t* d_depth, int n, int rows,
                                     uint16_t* d_packed_counts, mpc_basis_choice* d_packed_choices, void* stream);
mpc_status mpc_budget_allocate_floor_device(mpc_context* ctx, const uint32_t* d_profile, const uint16_t* d_counts, const uint8_t* d_floor,
                                            const uint8_t* d_must, long long n, const uint32_t* weights, int j, uint8_t* d_depth,
                                            uint16_t* d_out_counts, uint8_t* d_send, unsigned long long* d_totals, void* stream);

/* THE SESSION.  A delta session (mpc_delta_create) gets the map sent[t].  THE INVARIANT: after every successful budget call, a receiver
 * session that has applied every patch so far holds exactly -- byte for byte, in the context's flavour -- what mpc_decode_tiles_device
 * makes of the current frame's full records (mpc_encode_tiles_device's, by the delta encoder's contract) with every count cut to
 * min(count, sent[t]).  A sender-only feature: patches stay format version 1, mpc_patch_apply and every decoder read them unchanged.
 *
 * mpc_delta_encode_patch_budget: a patch of at most `budget` bytes.  Synchronous.
 *   1. mpc_delta_encode_patch's refusals, flags, key-frame rule and stages up to the records (frame, list, pursuit, scatter), and two
 *      more: budget < 40 (an empty patch) is MPC_ERR_ARGUMENT with nothing enqueued, and a session whose sent map is not valid -- the
 *      first budget call, a budget call after an unbudgeted call, after a failure behind the checks -- makes the call a key frame
 *   2. key frame: every tile is a candidate and must.  Else the owed-flags kernel and the flags -> list kernels make the candidates
 *   3. no candidates: the empty patch
 *   4. the candidates' pixels from the kept frame (the pack kernel) and their records from the store (the gather kernel) are an
 *      ordinary packed frame with its records; every tile a candidate: the frame and the store themselves.  F is its full container
 *      with its seek index, on job slot 0; all_bytes the length of the patch that carries F.  all_bytes <= budget: that patch is
 *      sent, sent = K for every candidate; on a session that owes nothing it is byte for byte mpc_delta_encode_patch's
 *   5. else the weights from F's index and the depth profile of the packed frame, once.  probe(j): the floor allocation, `send`
 *      compacted to a list, the records of the k candidates sent, cut to their depths, gathered into the packed frame of exactly
 *      those (mpc_delta_pack_geometry(k, 64); k = T: the whole frame's geometry and a key patch), the container job, mpc_patch_make;
 *      k = 0: the empty patch and no job.  size(j) is that patch's length
 *   6. probe(255) first (every must tile at depth 0 and nothing else); larger than the budget: MPC_ERR_ARGUMENT with both figures in
 *      the text, and the session is invalidated (the store has advanced): its next call is a key frame.  Then
 *      mpc_encode_image_budget's bisection: lo = -1 infeasible, hi = 255 feasible, at most nine probes, hi's patch kept from its probe
 *   7. commit: sent[t] = depth for every tile sent; the sequence advances as for mpc_delta_encode_patch
 * A KEY budget call's container is byte for byte mpc_encode_image_budget_device(frame, budget - 40)'s, with its lambda_index and probes.
 * info: tiles, changed, key (a key frame, or a patch sent as a key patch); candidates; sent_tiles; owed (after the call); lambda_index
 * (-1: everything fitted); probes; all_bytes; sse (the sum of P over the candidates at the returned patch's depths).
 * mpc_delta_encode and mpc_delta_encode_patch keep their behaviour; a successful check of theirs marks the sent map invalid (a flag,
 * no launch), so the next budget call is a key frame.
 * mpc_delta_sent: the map after the last successful budget call, with mpc_delta_changed's capacity rules (*n = tiles);
 * MPC_ERR_ARGUMENT on a session without a valid map. */
typedef struct mpc_rate_info {
    int tiles, changed, key, candidates, sent_tiles, owed, lambda_index, probes;
    size_t all_bytes;
    unsigned long long sse;
} mpc_rate_info;
mpc_status mpc_delta_encode_patch_budget(mpc_delta* d, const uint8_t* rgb, size_t row_stride, const double* quant, unsigned flags,
                                         size_t budget, uint8_t** patch, size_t* patch_bytes, mpc_rate_info* info);
mpc_status mpc_delta_sent(const mpc_delta* d, uint8_t* depth, int capacity, int* n);

/* ---- "-s" patch statistics, Compression.cpp:200-302 ----
 * The reference seeds one std::mt19937, and for every image draws `patches` origins x = rand() % (width - bs),
 * y = rand() % (height - bs), runs CalcMPDynamic on the Y, U and V patch with every quantiser 1.0 and feeds
 * intCoeff and deltaId of steps 0..count-1 to math::Stat::update (Welford, SimpleMatrix/src/covariance.cpp:5-25);
 * its text report is how Data/stats.txt and the variance tables s_varY/U/V (CompressedImage.cpp:17-122) were made.
 * Here the patches of one image are encoded in one launch of the tile encoder on ctx's device; the statistics are
 * updated on the host in the reference's order, so every double equals the reference's bit for bit. */
typedef struct mpc_patch_stats mpc_patch_stats;
mpc_status mpc_patch_stats_create(mpc_context* ctx, unsigned seed, mpc_patch_stats** out);
void mpc_patch_stats_destroy(mpc_patch_stats* s);
/* images narrower or lower than the block are skipped like Compression.cpp:233-236 (MPC_OK, nothing drawn);
 * width or height == block size is MPC_ERR_ARGUMENT (the reference divides by zero there). */
mpc_status mpc_patch_stats_add_image(mpc_patch_stats* s, const uint8_t* rgb, int width, int height, int patches);
/* out[3][2][K][5]: channel Y,U,V x {intCoeff, deltaId} x step x {N, min, max, mean, sumSq} */
mpc_status mpc_patch_stats_read(const mpc_patch_stats* s, double* out);
/* the report of Compression.cpp:275-301 as '\n'-terminated lines; release with mpc_free */
mpc_status mpc_patch_stats_report(const mpc_patch_stats* s, char** text, size_t* nbytes);
/* std::format("{}", v) of one double (shortest round-trip text), NUL terminated into buf[cap]; returns the length */
int mpc_format_double(double v, char* buf, int cap);

/* compressed::calculatePSNR (CompressedImage.h:57) */
double mpc_psnr(const uint8_t* original, const uint8_t* decoded, int width, int height);

/* ---- rate-distortion curves: Compression.cpp -n (:144-182) and -g (:303-350) without the container coming back in ----
 * createQuantizationTables (CompressedImage.cpp:124-166) without a context: quant[3*K], Y then U then V, what
 * mpc_context_create(K, block_size, bpp_allocation, ...) installs.  K 1..32, block size 1..8, bpp finite.  Host only. */
mpc_status mpc_quant_tables(int K, int block_size, double bpp_allocation, double* quant);

/* Squared reconstruction error of whole-frame records (tile t = tx*tiles_y + ty, what mpc_encode_tiles_device returns for
 * tile rows [0, tiles_y)) against the RGB frame they were encoded from (3*width bytes per row), all in device memory: exactly
 * calculatePSNR's sum (CompressedImage.cpp:343-357) between that frame and what mpc_decode_image reconstructs from the
 * container of these records.  The reconstruction is the decoder's (mp_decode_kernel; the context's fast flag selects the
 * flavour) with the quantiser steps the container header carries: quant (host [3*K], NULL = the context's tables) truncated to
 * u16 as writeCompressed stores them (:419-427), not the encoder's doubles.  *d_sse (u64) += the frame's sum (the caller zeroes
 * it); d_tile_sse[tiles] (u32, optional) = each tile's.  Asynchronous on `stream`. */
mpc_status mpc_distortion_device(mpc_context* ctx, const uint16_t* d_counts, const mpc_basis_choice* d_choices, const double* quant,
                                 const uint8_t* d_rgb, int width, int height, unsigned long long* d_sse, uint32_t* d_tile_sse,
                                 void* stream);

/* One frame (host, 3*width bytes per row) at n_levels quantiser tables quants[n_levels][3*K]: per level i
 *   nbytes[i]  the container's size; bytes[i] (bytes != NULL; mpc_free) the container, byte-identical to
 *              mpc_encode_image(ctx, rgb, width, height, quants + 3*K*i)
 *   sse[i]     (optional) the exact integer sum of squared differences between rgb and mpc_decode_image(bytes[i])
 *   psnr[i]    (optional) calculatePSNR's value from it, bit-identical to mpc_psnr (+inf for a lossless level)
 * Levels are pipelined: level i+1's tile encode runs while the host builds level i's code tables; the decoded frames never
 * exist.  The call uses container job slots 0..2 of the context (they must be idle) and leaves its quant tables, fast flag and
 * tile-encode workgroups as it found them.  On failure nothing is returned. */
mpc_status mpc_rate_distortion(mpc_context* ctx, const uint8_t* rgb, int width, int height, const double* quants, int n_levels,
                               size_t* nbytes, unsigned long long* sse, double* psnr, uint8_t** bytes);
/* The same with the frame already in device memory (3*width bytes per row, tightly packed). */
mpc_status mpc_rate_distortion_device(mpc_context* ctx, const uint8_t* d_rgb, int width, int height, const double* quants,
                                      int n_levels, size_t* nbytes, unsigned long long* sse, double* psnr, uint8_t** bytes);

/* ---- emphasis: budget, quality and rate encodes weigh tiles ("Encoder: emphasis") ----
 * The three encoders that cut a frame to a constraint minimise the plain squared error of the whole frame: every tile counts the same.
 * An emphasis map says where the bytes matter -- a face, the text under the cursor, a saliency network's output -- as one factor per
 * tile on the distortion term of the allocation.  Everything downstream (the depth cut, the container job, the patch, every decoder) is
 * untouched.  P, W, R, L[j], floor, must and the totals are the budget, quality and rate sections'; tile t = tx * tiles_y + ty as
 * everywhere.  Host and device agree bit for bit on everything defined here.
 *
 * EMPHASIS  e[t], one u8 per tile of the frame, four fractional bits: MPC_EMPHASIS_NEUTRAL = 16 is the factor 1, the range is
 * 1 ... MPC_EMPHASIS_MAX = 64 (1/16 ... 4).  A stored 0 is used as 1 and a value above 64 as 64 (the "count above K is used as K"
 * rule); no address ever comes from an emphasis value.
 * ALLOCATION AT j WITH EMPHASIS  J(t, n) = P[t][n] * e[t] * 4096 + L[j] * R[t][n] in u64; depth[t] = the smallest n that minimises J;
 * out_counts as in mpc_budget_allocate; totals[0] = the sum of the UNWEIGHTED P[t][depth[t]], the true squared error that
 * mpc_decode_image shows; totals[1] and [2] as there.  With e = 16 everywhere it is mpc_budget_allocate, bit for bit.
 * BOUNDS  P <= 64 * 3 * 255^2 = 12 484 800, hence P * 64 * 4096 <= 3.28e12 < 14 * 2^39 = 7.70e12, the cost of the cheapest record at
 * j = 255: there every depth is still 0, the budget search keeps its feasible end, and J stays below 2^63.
 * SWEEP WITH EMPHASIS  S[j][k] are exactly those totals at every j.  Scaling a tile's P by a positive constant leaves the optimality
 * argument intact: a tile's P at its minimiser does not fall as L rises, so S[j][0], the true squared error, still never falls along
 * the ladder, and mpc_quality_pick is used unchanged.  A quality target stays a promise about the frame's true error; emphasis only
 * decides where the remaining error lies.
 * FLOOR ALLOCATION WITH EMPHASIS  the rate section's, with the same J over R'.  Candidate i takes e[list[i]], list == NULL the
 * identity; a list entry outside [0, tiles) takes the neutral value.  totals[0] is unweighted.
 * MASK TO EMPHASIS  from a u8 mask at pixel resolution, width x height, row_stride >= width bytes a row, any alignment; the bytes
 * between rows are never read.  e[t] = lo + ((hi - lo) * m + 127) / 255, m the maximum of the mask over the pixels of tile t that lie
 * inside the frame; 1 <= lo <= hi <= 64.
 *
 * Host only, no context, safe on several threads; they define what the kernels compute.  emphasis: `tiles` bytes, NULL = neutral:
 *   mpc_budget_allocate_emphasis, mpc_budget_sweep_emphasis   mpc_budget_allocate's and mpc_budget_sweep's arguments and refusals
 *   mpc_budget_allocate_floor_emphasis   mpc_budget_allocate_floor's, and with a map: tiles >= 1, and n <= tiles where list is NULL
 *   mpc_emphasis_from_mask               emphasis[tiles of the geometry].  MPC_ERR_ARGUMENT: a null pointer, a geometry outside
 *                                        mpc_rate_distortion's, row_stride < width, lo or hi outside 1 <= lo <= hi <= 64
 * On the caller's buffers, asynchronous on `stream`, with their siblings' contract: ordered on the caller's stream, a capturing stream
 * refused with nothing enqueued, MPC_ERR_NO_DEVICE for a host-only context, the host forms' argument refusals:
 *   mpc_budget_allocate_emphasis_device, mpc_budget_sweep_emphasis_device, mpc_budget_allocate_floor_emphasis_device
 *                                        d_emphasis (and d_list): device memory, NULL = the sibling itself, the same kernel
 *   mpc_emphasis_from_mask_device        d_mask and d_emphasis in device memory; one pass over the mask
 *
 * mpc_encode_image_budget_emphasis[_device], mpc_encode_image_quality_emphasis[_device]: today's calls with a map (host form: host
 * memory, `tiles` bytes; _device: device memory) handed to every allocation and to the sweep.  NULL: byte for byte today's call, with
 * the same info.  The search, the step numbering, the refusals and "leaves the context as it found it" are those calls'; the budget
 * form still returns F untouched when |F| <= budget, and info->sse stays the true squared error of the result, so the quality form
 * still promises info->sse <= max_sse at the largest such j.  NOT promised, as today: a minimal byte count, or one monotone in the
 * constraint.
 *
 * mpc_delta_set_emphasis: the map (host memory, `tiles` bytes) is copied into the session's device memory and weighs every later
 * mpc_delta_encode_patch_budget until set again; NULL (tiles ignored) = none.  It does not invalidate the sent map: depths already sent
 * stay true.  MPC_ERR_ARGUMENT for a tile count that is not the session's; the session stays as it was.  mpc_delta_encode and
 * mpc_delta_encode_patch ignore it.  A KEY budget call's container is byte for byte
 * mpc_encode_image_budget_emphasis_device(frame, budget - 40, the same map)'s, with its lambda_index and probes. */
#define MPC_EMPHASIS_NEUTRAL 16
#define MPC_EMPHASIS_MAX 64
mpc_status mpc_budget_allocate_emphasis(const uint32_t* profile, const uint16_t* counts, const uint8_t* emphasis, long long tiles, int K,
                                        const uint32_t* weights, int j, uint8_t* depth, uint16_t* out_counts, uint64_t* totals /* [3] */);
mpc_status mpc_budget_sweep_emphasis(const uint32_t* profile, const uint16_t* counts, const uint8_t* emphasis, long long tiles, int K,
                                     const uint32_t* weights, uint64_t* totals /* [256 * 3] */);
mpc_status mpc_budget_allocate_floor_emphasis(const uint32_t* profile, const uint16_t* counts, const uint8_t* floor, const uint8_t* must,
                                              const uint8_t* emphasis, const int32_t* list, long long tiles, long long n, int K,
                                              const uint32_t* weights, int j, uint8_t* depth, uint16_t* out_counts, uint8_t* send,
                                              uint64_t* totals /* [4] */);
mpc_status mpc_emphasis_from_mask(const uint8_t* mask, int width, int height, size_t row_stride, int lo, int hi, uint8_t* emphasis);
mpc_status mpc_budget_allocate_emphasis_device(mpc_context* ctx, const uint32_t* d_profile, const uint16_t* d_counts, const uint8_t* d_emphasis,
                                               long long tiles, const uint32_t* weights, int j, uint8_t* d_depth, uint16_t* d_out_counts,
                                               unsigned long long* d_totals, void* stream);
mpc_status mpc_budget_sweep_emphasis_device(mpc_context* ctx, const uint32_t* d_profile, const uint16_t* d_counts, const uint8_t* d_emphasis,
                                            long long tiles, const uint32_t* weights, unsigned long long* d_totals /* [768] */, void* stream);
mpc_status mpc_budget_allocate_floor_emphasis_device(mpc_context* ctx, const uint32_t* d_profile, const uint16_t* d_counts,
                                                     const uint8_t* d_floor, const uint8_t* d_must, const uint8_t* d_emphasis,
                                                     const int32_t* d_list, long long tiles, long long n, const uint32_t* weights, int j,
                                                     uint8_t* d_depth, uint16_t* d_out_counts, uint8_t* d_send, unsigned long long* d_totals,
                                                     void* stream);
mpc_status mpc_emphasis_from_mask_device(mpc_context* ctx, const uint8_t* d_mask, int width, int height, size_t row_stride, int lo, int hi,
                                         uint8_t* d_emphasis, void* stream);
mpc_status mpc_encode_image_budget_emphasis(mpc_context* ctx, const uint8_t* rgb, const uint8_t* emphasis, int width, int height,
                                            const double* quant, size_t budget, int index_interval, uint8_t** bytes, size_t* nbytes,
                                            uint8_t** index, size_t* index_bytes, uint8_t* depth, mpc_budget_info* info);
mpc_status mpc_encode_image_budget_emphasis_device(mpc_context* ctx, const uint8_t* d_rgb, const uint8_t* d_emphasis, int width, int height,
                                                   const double* quant, size_t budget, int index_interval, uint8_t** bytes, size_t* nbytes,
                                                   uint8_t** index, size_t* index_bytes, uint8_t* depth, mpc_budget_info* info);
mpc_status mpc_encode_image_quality_emphasis(mpc_context* ctx, const uint8_t* rgb, const uint8_t* emphasis, int width, int height,
                                             const double* quant, unsigned long long max_sse, int index_interval, uint8_t** bytes,
                                             size_t* nbytes, uint8_t** index, size_t* index_bytes, uint8_t* depth, mpc_quality_info* info);
mpc_status mpc_encode_image_quality_emphasis_device(mpc_context* ctx, const uint8_t* d_rgb, const uint8_t* d_emphasis, int width, int height,
                                                    const double* quant, unsigned long long max_sse, int index_interval, uint8_t** bytes,
                                                    size_t* nbytes, uint8_t** index, size_t* index_bytes, uint8_t* depth,
                                                    mpc_quality_info* info);
mpc_status mpc_delta_set_emphasis(mpc_delta* d, const uint8_t* emphasis /* host, tiles bytes, or NULL */, int tiles);

/* ---- group: a group of frames to one byte budget or one quality ("Encoder: a group of frames") ----
 * A burst, a tile mosaic, a short clip: `frames` frames of one geometry and one constraint for all of them.  The squared error of a cut
 * is additive over tiles, whichever frame a tile belongs to, so ONE multiplier across all tiles of all frames gives the equal-slope
 * allocation across frames as well as within them: a flat frame gives its bytes to a textured one.  P, W, R, L[j], J, the allocation at
 * j, the sweep and the pick are the budget and quality sections', e[t] the emphasis section's, unchanged.  Host and device agree bit for
 * bit on everything defined here.
 *
 * A GROUP is `frames` frames, T tiles each, K the context's, 1 <= frames <= MPC_GROUP_MAX_FRAMES = 64.  Records, profile, depth and cut
 * counts are FRAME-MAJOR: tile t of frame f is tile f * T + t of every array (what mpc_encode_batch_device writes for whole frames).
 * WEIGHTS  weights[f * 3K + ch * K + i]: frame f's own, mpc_budget_weights of frame f's full container's index.
 * EMPHASIS  NULL, or frames * T bytes, frame-major; a neutral byte is the plain allocation, as in the emphasis section.
 * GROUP ALLOCATION AT j  for every frame f exactly mpc_budget_allocate_emphasis of frame f's profile, counts, weights and map slice at
 * j; totals[3 * f + k] are that frame's totals.
 * GROUP SWEEP  S[j][k] = the sum over f of mpc_budget_sweep_emphasis of frame f: 768 u64 words.  A sum of sequences that never fall is one:
 * mpc_quality_pick is used unchanged.
 *
 * Host only, no context, safe on several threads; they define what the kernels compute:
 *   mpc_budget_allocate_group   depth[frames * T] and out_counts[3 * frames * T]: each NULL or room for that; totals[3 * frames]
 *   mpc_budget_sweep_group      totals[768]
 *   mpc_sse_for_psnr_group      *max_sse = the largest s in 0 ... 195075 * 64 * tiles * frames whose PSNR over frames * width * height
 *                               pixels, by mpc_psnr's formula, is >= psnr: the same binary search; with frames = 1 it is mpc_sse_for_psnr
 * Their refusals are mpc_budget_allocate_emphasis's, mpc_budget_sweep_emphasis's and mpc_sse_for_psnr's, and MPC_ERR_ARGUMENT for frames
 * outside 1 ... 64.
 *
 * mpc_budget_allocate_group_device, mpc_budget_sweep_group_device: the two on the caller's buffers (device memory; d_emphasis NULL or
 * device memory) with weights[frames * 3K] in HOST memory, read before the call returns (they travel in the kernels' arguments, eight
 * frames a launch): d_depth[frames * T], d_out_counts[3 * frames * T], d_totals[3 * frames] resp. d_totals[768] (u64; zeroed on `stream`
 * first).  Asynchronous on `stream`, with their siblings' contract: ordered on the caller's stream, a capturing stream refused with
 * nothing enqueued, MPC_ERR_NO_DEVICE for a host-only context; MPC_ERR_ARGUMENT for a null pointer, frames outside 1 ... 64, T < 1 or
 * 3 * frames * T >= 2^31, j outside 0 ... 255.
 *
 * mpc_encode_images_budget[_device]: containers of the frames (host: pointers to host frames of 3 * width bytes a row; _device: pointers,
 * in host memory, to tightly packed device frames) of at most `budget` bytes together.  Synchronous.
 *   1. the whole group is pursued in one launch (mpc_encode_batch_device); the records stay on the device
 *   2. every frame's full container F_f with its seek index is made
 *   3. sum |F_f| <= budget: the F_f are returned, byte for byte mpc_encode_images; lambda_index = -1, probes = 0, every depth K
 *   4. else the weights and the depth profile of every frame are made, once each
 *   5. size(j) = the sum over f of the container of frame f's cut counts at j: one group allocation and n container jobs
 *      (a probe whose sum is above the budget after fewer frames stops there; size(255) is always made whole)
 *   6. size(255) > budget: MPC_ERR_ARGUMENT, the budget and size(255) in the text
 *   7. mpc_encode_image_budget's bisection between -1 and 255; probes counts multipliers, not jobs
 *   8. hi's containers are returned, kept from their probe
 * mpc_encode_images_quality[_device]: the frames as the containers of the group allocation at the largest multiplier whose squared
 * error over the whole group is at most max_sse: the same start, the weights and profiles, one group sweep, the pick (j = -1:
 * MPC_ERR_ARGUMENT, max_sse and S[0][0] in the text), the group allocation at j, n container jobs; the frames' totals at j are checked
 * against S[j].  What mpc_encode_image_quality promises and does not promise holds for the group's sums.
 * bytes[n], nbytes[n]: the containers (mpc_free each).  index_interval < 0: no index, `indexes` and `index_bytes` may be NULL; otherwise
 * indexes[f] (mpc_free) is byte for byte mpc_container_index2(bytes[f], ..., interval, MPC_INDEX_EXPANDED).  depth: NULL, or host room for
 * n * T bytes, frame-major.  emphasis: NULL or n * T bytes (host form: host memory; _device: device memory).  frame_info[n]: the single
 * call's struct for each frame, lambda_index and probes repeated (a frame's min_sse is its own allocation at multiplier 0); info: the
 * sums over the frames, lambda_index and probes once.
 * WITH n_frames = 1 BOTH CALLS RETURN BYTE FOR BYTE WHAT mpc_encode_image_budget[_emphasis] AND mpc_encode_image_quality[_emphasis]
 * RETURN, info included.
 * Refusals and side effects are the single-frame calls', with nothing enqueued, and MPC_ERR_ARGUMENT for n_frames outside 1 ... 64, a
 * null frame pointer and 3 * n * T >= 2^31.  On failure nothing is returned, the slots are idle and the context is as it was.  The
 * staging is the single calls', grown for the group; a group that does not fit in device memory returns that allocation's status.
 * Frames of different sizes, a group budget for the delta stream and probes that overlap are not built. */
#define MPC_GROUP_MAX_FRAMES 64
mpc_status mpc_budget_allocate_group(const uint32_t* profile, const uint16_t* counts, const uint8_t* emphasis, int frames, long long tiles, int K,
                                     const uint32_t* weights /* [frames][3K] */, int j, uint8_t* depth, uint16_t* out_counts,
                                     uint64_t* totals /* [frames][3] */);
mpc_status mpc_budget_sweep_group(const uint32_t* profile, const uint16_t* counts, const uint8_t* emphasis, int frames, long long tiles, int K,
                                  const uint32_t* weights /* [frames][3K] */, uint64_t* totals /* [256 * 3] */);
mpc_status mpc_sse_for_psnr_group(double psnr, int width, int height, int frames, uint64_t* max_sse);
mpc_status mpc_budget_allocate_group_device(mpc_context* ctx, const uint32_t* d_profile, const uint16_t* d_counts, const uint8_t* d_emphasis,
                                            int frames, long long tiles, const uint32_t* weights /* host, [frames][3K] */, int j,
                                            uint8_t* d_depth, uint16_t* d_out_counts, unsigned long long* d_totals /* [frames][3] */,
                                            void* stream);
mpc_status mpc_budget_sweep_group_device(mpc_context* ctx, const uint32_t* d_profile, const uint16_t* d_counts, const uint8_t* d_emphasis,
                                         int frames, long long tiles, const uint32_t* weights /* host, [frames][3K] */,
                                         unsigned long long* d_totals /* [768] */, void* stream);
mpc_status mpc_encode_images_budget(mpc_context* ctx, const uint8_t* const* frames, const uint8_t* emphasis, int n_frames, int width, int height,
                                    const double* quant, size_t budget, int index_interval, uint8_t** bytes, size_t* nbytes,
                                    uint8_t** indexes, size_t* index_bytes, uint8_t* depth, mpc_budget_info* frame_info,
                                    mpc_budget_info* info);
mpc_status mpc_encode_images_budget_device(mpc_context* ctx, const uint8_t* const* d_frames, const uint8_t* d_emphasis, int n_frames, int width,
                                           int height, const double* quant, size_t budget, int index_interval, uint8_t** bytes,
                                           size_t* nbytes, uint8_t** indexes, size_t* index_bytes, uint8_t* depth,
                                           mpc_budget_info* frame_info, mpc_budget_info* info);
mpc_status mpc_encode_images_quality(mpc_context* ctx, const uint8_t* const* frames, const uint8_t* emphasis, int n_frames, int width, int height,
                                     const double* quant, unsigned long long max_sse, int index_interval, uint8_t** bytes, size_t* nbytes,
                                     uint8_t** indexes, size_t* index_bytes, uint8_t* depth, mpc_quality_info* frame_info,
                                     mpc_quality_info* info);
mpc_status mpc_encode_images_quality_device(mpc_context* ctx, const uint8_t* const* d_frames, const uint8_t* d_emphasis, int n_frames,
                                            int width, int height, const double* quant, unsigned long long max_sse, int index_interval,
                                            uint8_t** bytes, size_t* nbytes, uint8_t** indexes, size_t* index_bytes, uint8_t* depth,
                                            mpc_quality_info* frame_info, mpc_quality_info* info);

/* ---- patch index: a patch that carries its container's seek index ("Delta stream") ----
 * The receiver of a version-1 patch parses the container's entropy codes on the host, serially: the cost follows the bytes.  A
 * version-2 patch brings the seek index of its container along, and mpc_patch_apply hands container and index to the sequence
 * decoder's indexed route, which parses the codes on the device.
 *
 * THE FORMAT, version 2, little endian:
 *    0 "MPCP" | 4 u16 version = 2 | 6 u16 flags (bit 0 = key) | 8 u32 width | 12 u32 height | 16 u32 sequence |
 *   20 u32 n | 24 u32 list_bytes | 28 u32 index_bytes (> 0) | 32 u64 container_bytes | 40 the list | the container | the index
 * exactly 40 + list_bytes + container_bytes + index_bytes long; list and container as in version 1.  The forms are key and tile: there
 * is no version-2 empty patch, and a patch without an index is written as version 1.  A version-2 header with index_bytes == 0 is
 * refused, as is a version-1 header whose word at 28 is not 0.  The index section is a version-1 seek-index blob ("MPIX", the seek
 * index section above), but the patch parser checks its framing alone: the index is a hint, a patch whose index section is garbage
 * is a valid patch, and applying it gives the pixels of the patch without it.  The section starts wherever the list and the
 * container end, at any alignment: a reader copies it or reads it bytewise.
 * mpc_patch_info and mpc_patch_tiles accept version 2 and report what they report for the stripped patch.
 *
 * Host only, no context, safe on several threads; outputs are mpc_free's:
 *   mpc_patch_index         validates as mpc_patch_info does; the index section's offset from `bytes` and its size, (0, 0) for version 1
 *   mpc_patch_make_indexed  mpc_patch_make with an index section: index_bytes == 0 writes the version-1 blob; MPC_ERR_ARGUMENT for an
 *                           index given for an empty patch, index_bytes >= 2^32, or index == NULL with index_bytes != 0.  The bytes
 *                           are copied as they are
 *   mpc_patch_strip_index   the version-1 patch, byte for byte: a version-1 patch's own bytes
 *   mpc_patch_add_index     what a sender that attaches the index does.  Any index present is stripped.  Where the patch has a
 *                           container of at least max(index_min_bytes, 1) bytes and mpc_container_index(container, interval) succeeds
 *                           with an index that is not "serial only", that blob is appended and the patch is version 2; otherwise the
 *                           version-1 patch comes back.  interval: mpc_container_index's rules (0 = the default, else 32 ... 65536)
 * A refused patch is MPC_ERR_BITSTREAM and nothing is written.
 *
 * THE SENDER, mpc_delta_encode_patch_indexed: mpc_delta_encode_patch's refusals, flags, stages and session effects -- the session
 * advances identically whichever of mpc_delta_encode, mpc_delta_encode_patch and this call is used, in any mix -- plus
 * mpc_delta_encode's refusal of an interval that is none.  index_interval < 0: exactly mpc_delta_encode_patch.  Else the result is
 * byte for byte mpc_patch_add_index(P, index_interval, index_min_bytes) of the patch P mpc_delta_encode_patch returns for the call.
 * The index comes from the container job's entropy stage (a key patch: the store's job; a tile patch: the packed frame's); the
 * finished container is parsed only where the frame takes the host entropy route, as for every indexed encoder.  index_min_bytes
 * leaves small patches at version 1: below some size the device parse's fixed cost (the host's tables for 1 + 6K streams and about a
 * dozen launches) exceeds the serial parse, and the index adds about a tenth to the bytes.
 *
 * THE RECEIVER: mpc_patch_apply decodes a version-2 patch's container as mpc_decode_images_indexed_device does with n = 1 and the
 * patch's index section; staging, the list upload, the unpack kernel and a key patch's copy are version 1's.  Pixels, statuses and
 * error texts are those of applying the stripped patch, and so is the atomicity rule.
 *   mpc_patch_last_route  of the last successful apply: 0 = the codes were parsed on the device; 1 = serial (a version-1 patch, or the
 *                         decoder refused the index); -1 = nothing was decoded (an empty patch, no apply yet, p == NULL) */
mpc_status mpc_patch_index(const uint8_t* bytes, size_t nbytes, size_t* index_offset, size_t* index_bytes);
mpc_status mpc_patch_make_indexed(int width, int height, uint32_t sequence, int key, const int32_t* tiles, int n, const uint8_t* container,
                                  size_t container_bytes, const uint8_t* index, size_t index_bytes, uint8_t** bytes, size_t* nbytes);
mpc_status mpc_patch_add_index(const uint8_t* patch, size_t nbytes, int interval, size_t index_min_bytes, uint8_t** out, size_t* out_bytes);
mpc_status mpc_patch_strip_index(const uint8_t* patch, size_t nbytes, uint8_t** out, size_t* out_bytes);
mpc_status mpc_delta_encode_patch_indexed(mpc_delta* d, const uint8_t* rgb, size_t row_stride, const double* quant, unsigned flags,
                                          int index_interval, size_t index_min_bytes, uint8_t** patch, size_t* patch_bytes,
                                          mpc_delta_info* info);
int        mpc_patch_last_route(const mpc_patch_decoder* p);

/* ---- test entry points ----
 * These exist for the tests of the pursuit screen's tables (tests/test_screen_cases.py, tests/test_gpu_screen_tables.py) and are
 * on no product path.  The screen decides nothing: a wrong Gram entry, a wrong filter tile or a bound that does not
 * hold changes no record until a contest happens to fall inside the error, so these three are read back and probed directly;
 * the kernel's key tracking is probed the same way (mpc_debug_track_probe_device, tests/test_gpu_track_keys.py).
 * Every entry checks its arguments before it touches memory: MPC_ERR_ARGUMENT for a null pointer, a channel outside 0 ... 2, a
 * block outside 0 ... num_base - 1, n outside 1 ... 16 or a rectangle outside the table; MPC_ERR_NO_DEVICE for a host-only context.
 *
 * The resident Gram table of `channel` is [num_base + detail_rows][num_base * 64] floats: row sel = base row sel (sel < num_base)
 * or detail row sel - num_base of the channel; column 64 * blk + row = row `row` of DetailBasis[blk] of the channel (pad rows: 0).
 * Copies rows [sel_begin, + sel_count) x columns [col_begin, + col_count) to the dense d_out[sel_count][col_count] on `stream`. */
mpc_status mpc_debug_copy_gram_device(mpc_context* ctx, int channel, int sel_begin, int sel_count, int col_begin, int col_count,
                                      float* d_out, void* stream);
/* The Gram kernel on the caller's own device arrays: d_base[num_base][64], d_detail[rows][64], d_block_rows[num_base] (<= 64 each),
 * d_block_row_off[num_base] (first detail row of each block), d_shadow[rows] (1 = the row's column is left 0), n_sel = num_base +
 * rows; d_gram[n_sel][num_base * 64] (16-byte aligned) as above, rows beyond n_sel are not written.  Asynchronous on `stream`. */
mpc_status mpc_debug_gram_device(const double* d_base, const double* d_detail, const int32_t* d_block_rows, const int32_t* d_block_row_off,
                                 const uint8_t* d_shadow, int num_base, int n_sel, float* d_gram, void* stream);
/* The uploaded split-bf16 filter tiles as the pursuit kernel reads them, to host memory: channel = -1: the 32 base tiles
 * (host_out[32 * 2048], block ignored); channel 0 ... 2: the 4 tiles of DetailBasis[block] of that channel (host_out[4 * 2048]). */
mpc_status mpc_debug_copy_filter_tiles(mpc_context* ctx, int channel, int block, uint16_t* host_out);
/* Host only, no context: the function that makes those tiles.  rows[nrows][64] doubles, nrows <= 16 * tiles, tiles 1 ... 64;
 * every element x becomes hi = bf16(float(x)), lo = bf16(float(x) - hi), round to nearest even, at
 *   out[((tile*4 + 2*kk + part)*64 + lane)*8 + j]   (part 0 = hi, 1 = lo)
 * of row tile*16 + (lane & 15), pixel 32*kk + 8*(lane >> 4) + j (k_order 0) or 16*pos(lane >> 4) + 8*kk + j with pos = 0, 1, 3, 2
 * (k_order 1, the pursuit kernel's).  out[tiles * 2048].  A row that is bit for bit an earlier row or its negation is left zero
 * and marked in shadow[nrows] (optional); so are the rows from nrows on (unmarked). */
mpc_status mpc_filter_tiles(const double* rows, int nrows, int tiles, int k_order, uint16_t* out, uint8_t* shadow);
/* One wave of the pursuit's screen on n (1 ... 16) residual vectors d_vectors[n][64] (doubles, 16-byte aligned): the B operands as
 * the kernel's phase (2a) makes them (f64 -> f32, hi / lo bf16, |r~|, E), the six-MFMA tile product over the 32 resident base tiles
 * and the 4 resident tiles of DetailBasis[block] of `channel`.  d_approx[n][576] (16-byte aligned): [16*tile + 4*h + v] = the
 * approximation of base row 0 ... 511, then of block row 0 ... 63; d_bound[n] = E.  Asynchronous on `stream`. */
mpc_status mpc_debug_screen_probe_device(mpc_context* ctx, int channel, int block, const double* d_vectors, int n, float* d_approx,
                                         float* d_bound, void* stream);
/* One wave of the pursuit's key tracking ("keys"), needing no dictionary: the kernel's own functions on the caller's
 * bit patterns, once as the definition (one value after the other) and once grouped (four values in nine instructions), which
 * must agree bit for bit.  Lane l (row h = l >> 4) reads d_row_bits[l][144] (16-byte aligned): [4*tile + v] is taken for the
 * approximation of tile 0 ... 31 of the base rows, then of tile 0 ... 3 of DetailBasis[0], and tracked with the 7-bit row codes
 * 4*tile + v; and d_pair_bits[l][16] (16-byte aligned): [4*t + v] is taken for P of row 16*t + 4*h + v of one pair whose bound is
 * `bound`, whose block has `rows` (1 ... 64) rows and whose number is `pair` (0 ... 31): keys of |P| + bound with the 9-bit codes
 * pair << 4 | t << 2 | v, zero for the pad rows (row >= rows of rows 62 and 63).  Values must be finite.
 * d_out[l][14]: base keys k1, k2 by the definition, k1, k2 grouped; block keys likewise; pair k1, k2, largest |P| by the
 * definition, then grouped.  Asynchronous on `stream`. */
mpc_status mpc_debug_track_probe_device(mpc_context* ctx, const uint32_t* d_row_bits, const uint32_t* d_pair_bits, float bound, int rows,
                                        int pair, uint32_t* d_out, void* stream);
/* The persistent pursuit kernel's pair scratch ("pairs"), filled and read back around a pursuit
 * (tests/test_gpu_pair_drift.py).  A wave of the kernel (number blockIdx.x * waves per workgroup + wave) keeps, per slot (16) and pair
 * (32): 64 floats P (the kept approximations of the block's rows; pad rows 0), 2 words of bookkeeping (word 0 = block | rows << 9 |
 * first dictionary index << 16, word 1 unused) and 1 float E (the bound on |P - exact projection|).  For waves [wave_begin,
 * wave_begin + wave_count): fill = 1 first sets every 32-bit word of the three arrays to fill_word (fill = 0: nothing is written);
 * then the three arrays are copied to host_p[wave_count][16][32][64], host_meta[wave_count][16][32][2], host_e[wave_count][16][32].
 * Synchronous, like mpc_calc_mp_batch: waits for the device and holds off pursuit launches of the process meanwhile.  A batch of at
 * most 16 vectors of mpc_calc_mp_batch runs in one workgroup on one of waves 0 ... 11, vector s in slot s.
 * MPC_ERR_ARGUMENT: null context or output, fill other than 0 / 1, waves outside 0 ... 16 * workgroups of the scratch (one workgroup
 * per compute unit); MPC_ERR_NO_DEVICE for a host-only context; nothing is written then. */
mpc_status mpc_debug_pair_scratch(mpc_context* ctx, int wave_begin, int wave_count, int fill, uint32_t fill_word, float* host_p,
                                  uint32_t* host_meta, float* host_e);

#ifdef __cplusplus
}
#endif
#endif /* MPCODEC_H */
