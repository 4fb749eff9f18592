// mp_device.h -- product: device-side data layout and launchers of the MI355X (gfx950) quantized matching-pursuit tile
// encoder and of the stages behind it.
//
//   mp_pursuit.hip   the PERSISTENT pursuit kernel (the product's path): one launch runs all K steps of every tile-channel of a
//                    batch on chip -- LDS-resident dictionary, split-bf16 MFMA screen with a proven bound, Gram-updated detail
//                    blocks, exact evaluation of the survivors in the reference's arithmetic (PursuitArgs, launch_pursuit)
//   mp_streams.hip   stream assembly: the records -> the container's 6K symbol streams, live symbols only (StreamArgs)
//   mp_entropy.hip   the per-symbol work of the entropy stage: run lengths, histograms, first appearances, code writing (EntropyArgs)
//   mp_unpack.hip    the decoder's mirror of those two: run-length expansion and DC sums of coded streams (UnpackArgs)
//   mp_parse.hip     the entropy codes of a container undone chunk by chunk from a seek index (ParseArgs)
//   mp_scan.hip      that seek index's checkpoints found by a scan over every bit position of a stream (ScanArgs)
//   mp_budget.hip    rate control: a tile's squared error at every depth, the depth that minimises distortion + multiplier * rate,
//                    and that allocation's totals at all 256 multipliers in one launch
//   mp_rate.hip      a delta stream to a byte budget: owed flags, the records gather with a cut, the allocation with a floor
//   mp_kernels.hip   the decoder, the symbol histogram, and the product's own cross-check of the tile encoder: a STEP-SYNCHRONOUS
//                    pursuit that correlates every row exactly (a short sequence of kernels per MP step over the active
//                    tile-channels: init, fill, base sweep, detail sweep, finish, update), behind MPC_PATH=steps / MPC_FILTER=0
// The step-synchronous kernels' layout follows (Workspace, enqueue_pursuit); the persistent kernel's is further down.
#pragma once
#include <cstddef>
#include <cstdint>

namespace mpc {

constexpr int kHistBins = 8192;
constexpr int kMaxDeviceK = 32;
constexpr int kMaxParts = 8;            // base sweep can be split over up to 8 atom ranges per tile-channel group
constexpr int kChunkItems = 64;         // items (tile-channels) a wave processes per loaded detail block
constexpr int kNumBuckets = 3 * 512;    // (channel, block) buckets, block < 510
constexpr int kBaseFilterTiles = 32;    // 16-row tiles of the filter copy of the base dictionary (512 rows)
constexpr int kBlockFilterTiles = 4;    // ... of one detail block (62 | 63 rows, padded to 64)
constexpr int kMaxRowParts = 4;         // a detail block's 62/63 rows can be split over up to 4 waves

struct DictDevice {
    const double* base;              // [base_rows_padded + 1][64] row-major, zero rows after num_base
    int num_base;                    // 510
    int base_rows_padded;
    const double* detail;            // [3][detail_rows][64] row-major (+1 zero row at the very end)
    const float* base32;             // the same two, rounded to float (the `...Fast` flavour)
    const float* detail32;
    long long detail_rows;           // rows per channel (31 622)
    const int32_t* block_rows;       // [num_base]
    int block0_rows;                 // block_rows[0] (host copy)
    const int32_t* block_row_off;    // [num_base+1]
};

// Per-batch device workspace (all device pointers). cap = max tile-channels per batch.
struct Workspace {
    int cap;
    double* r;                       // [cap][64] residuals
    double* part_val;                // [cap][kMaxParts] best projection of each base atom range
    int* part_idx;                   // [cap][kMaxParts]
    double* cand0_val;               // [cap] best projection on DetailBasis[0] (if unlocked)
    int* cand0_row;                  // [cap]
    float* approx_max;               // [cap] filter pass: largest approximate projection over base rows + block 0
    int* prev_id;                    // [cap]
    int* nblk;                       // [cap] entries in blk_list
    int* extra_rows;                 // [cap] rows appended after the base part (duplicates included)
    unsigned* swept;                 // [cap]
    uint16_t* blk_list;              // [cap][32] chosen base atoms in order: bits 0-8 atom, 9-14 rows of its block, 15 = repeat
    int* item_slot;                  // [cap][32] bucket slot of each blk_list entry for the current step
    int* out_index;                  // [cap] record index in the low 30 bits, channel in the top 2
    int* act[2][3];                  // [cap] active tile-channels per channel (ping-pong)
    unsigned* counters;              // [16]: [cur*3+ch] = active count; 6 = chunk cursor; 7 = n_chunks; 8 = n_items
    unsigned* bucket_count[2];       // [kNumBuckets] items per (channel, block) for this / the next step
    unsigned* bucket_cursor;         // [kNumBuckets]
    int* chunks;                     // [max_chunks][4] = bucket, begin, end, 0
    int* items;                      // [max_items] tile-channel of each item
    double* cand_val;                // [max_items][kMaxRowParts] best projection of the item's block, per row range
    int* cand_row;                   // [max_items][kMaxRowParts]
    double* upd_coeff;               // [cap] finish -> update: coefficient of the chosen atom (0 = no update)
    int* upd_sel;                    // [cap] ~idx for a base atom, row index into `detail` otherwise
    long long max_items;
    int max_chunks;
};

// A launch over a few frames that lie anywhere (the frame pipeline's groups): frame f of the launch is read at rgb[f] and its tile
// `tile` (stripe order) writes record first[f] + tile.  n == 0: the strided form (rgb + f * frame_stride, records back to back).
// The kernel reads either form in its refill as PursuitArgs::frame_rgb / frame_first; with a table the records are in stripe
// order (out_tile_rows == 0).
constexpr int kFrameTable = 4;
struct FrameTable {
    int n;
    int first[kFrameTable];
    const uint8_t* rgb[kFrameTable];
};

struct FrameInput {
    const uint8_t* rgb;              // device, row-major, 3 B/pixel (img::image<rgb>, image.h:123-131)
    int width, height;
    long long row_stride;
    int frames;
    long long frame_stride;
    FrameTable table;                // n != 0: n == frames, and rgb / frame_stride are not read
    int tile_row_begin, tile_rows, tiles_x;
    int out_tile_rows;               // 0: records in stripe order (tile tx * tile_rows + ty - tile_row_begin); > 0: in the order of a
                                     // whole frame of this many tile rows (tx * out_tile_rows + ty): stripes encoded one by one
                                     // land where one launch over the frame would put them
    // vector mode (matching::CalcMPDynamic on caller vectors): vec_in != nullptr
    const double* vec_in;            // [n][64]
    int vec_channel;
};

struct Outputs {
    uint16_t* counts;                // [records]
    uint32_t* choices;               // [records][K]  lo16 = deltaId, hi16 = intCoeff
    double* energy;                  // [records] or null
    uint32_t* swept;                 // [records] or null
};

struct HistParams {
    const uint16_t* counts;          // [tiles][3]
    const uint32_t* choices;         // [tiles][3][K]
    long long tiles;
    int K;
    uint32_t* hist;                  // [(1 + 6K)][8192]
};

// Enqueue the whole K-step pursuit for the tile-channels [tc_begin, tc_begin + n) of the input on `stream`.
// Tile-channel numbering: tc = unit*3 + ch, unit = frame*tiles_per_frame_stripe + tx*tile_rows + (ty - begin)
// (vector mode: tc = vector index, channel fixed).  Returns hipError_t as int.  No host synchronisation,
// no allocation.
// base_events: optional array of 2*K hipEvent_t (as void*) recorded right before / after each base-sweep launch
// (live per-kernel timing for bench.py's roofline); nullptr = none.
int enqueue_pursuit(const DictDevice& dict, const Workspace& ws, const FrameInput& in, const Outputs& out,
                    const double* quant_dev, int K, long long tc_begin, int n, int parts, int row_parts, int sweep_waves,
                    void* stream, void** base_events);

int launch_histogram(const HistParams& p, void* stream);

// Decoder: FromCoeffsDynamic + RGBFromYUV for whole tiles.
struct DecodeParams {
    const uint16_t* counts;          // [tiles][3], tile t = tx*tiles_y + ty (the reference's visiting order)
    const uint32_t* choices;         // [tiles][3][K]
    const double* quant;             // [3][K] (device)
    int K;
    int width, height, tiles_x, tiles_y;
    uint8_t* rgb;                    // [height][width][3] (device)
    int* error_flag;                 // set to 1 if a record indexes outside its dynamic dictionary
    int fast;                        // != 0: FromCoeffsDynamicFast (float)
};
int launch_decode(const DictDevice& dict, const DecodeParams& p, void* stream);
// The same for the tiles a pixel rectangle touches (mp_decode_window_kernel): p.rgb receives the rectangle alone, rect_h rows of
// rect_w pixels tightly packed; p.counts / p.choices are the whole frame's, of which only the tiles [tx0, tx1) x [ty0, ty1) are read.
// The caller guarantees 0 <= rect_x, rect_x + rect_w <= p.width, the same for y, and rect_w, rect_h >= 1.
struct DecodeWindow {
    int rect_x, rect_y, rect_w, rect_h;
    int tx0, ty0, tx1, ty1;
};
int launch_decode_window(const DictDevice& dict, const DecodeParams& p, const DecodeWindow& w, void* stream);
// A view (mp_decode_view_kernel): the window's tiles reconstructed from the first `steps` records of every tile-channel -- the
// dynamic dictionary built from those alone -- and reduced by c = 1 << scale_log2: p.rgb receives ceil(rect_h / c) rows of
// ceil(rect_w / c) pixels, each the rounded mean (sum + n / 2) / n of the stored 8-bit values of its cell's n pixels that lie inside
// the rectangle.  The caller guarantees what launch_decode_window asks for, steps >= 1, 0 <= scale_log2 <= 3 and rect_x, rect_y
// multiples of c (a cell then never crosses a tile, and its first pixel lies inside the rectangle if any of it does).
struct DecodeView {
    int steps, scale_log2;
};
int launch_decode_view(const DictDevice& dict, const DecodeParams& p, const DecodeWindow& w, const DecodeView& v, void* stream);

// distortion (mp_kernels.hip: mp_distortion_kernel): the decode kernel's reconstruction compared with the original frame
struct DistortionParams {
    const uint16_t* counts;          // [tiles][3], tile t = tx*tiles_y + ty
    const uint32_t* choices;         // [tiles][3][K]
    const double* quant;             // [3][K] (device), the values the container header carries
    int K;
    int width, height, tiles_x, tiles_y;
    const uint8_t* original;         // [height][width][3] (device)
    unsigned long long* sse;         // += sum over the frame of dr^2 + dg^2 + db^2
    uint32_t* tile_sse;              // [tiles] or null: each tile's sum
    int fast;                        // != 0: FromCoeffsDynamicFast (float)
};
int launch_distortion(const DictDevice& dict, const DistortionParams& p, void* stream);

// ---- persistent pursuit (mp_pursuit.hip): one launch runs all K steps of every tile-channel of a batch ----
constexpr int kMaxPairs = 32;           // (tile-channel, unlocked block other than DetailBasis[0]) pairs a tile-channel can hold (< K)

struct PursuitArgs {
    // dictionary
    const double* base;              // [512][64]
    const double* detail[3];         // per channel [detail_rows][64]
    const uint16_t* base_tiles;      // [kBaseFilterTiles][2048], k order 1 (host_dictionary.h: filter_tiles)
    const uint16_t* block_tiles[3];  // per channel [num_base][kBlockFilterTiles][2048], k order 1
    const float* gram[3];            // per channel [num_base + detail_rows][gram_stride]
    long long gram_stride;           // num_base * 64
    const int32_t* block_rows;
    const int32_t* block_row_off;
    const double* quant;             // [3][K] (device)
    int K, num_base, rows0;
    // float flavour (`...Fast`): the same dictionary rounded to float, row layout as base / detail; fast != 0 selects it
    const float* base32;
    const float* detail32[3];
    int fast;
    // One launch covers all channels with `workgroups` workgroups (one per CU).  Every WAVE works on one channel at a time: luma
    // first, and once a channel's queue is dry the wave moves on to the next channel that has work (mp_pursuit.hip: channel
    // switch), so a channel's last long tile-channels drain beside the next channel's work instead of beside idle SIMDs.
    int workgroups;
    // input: tile mode (rgb) or vector mode (vec_in != nullptr: CalcMPDynamic on caller vectors of channel vec_channel)
    const uint8_t* frame_rgb[kFrameTable];   // frame f at frame_rgb[min(f, kFrameTable - 1)] + f * frame_stride ...
    int frame_first[kFrameTable];            // ... and its records moved by frame_first[min(f, kFrameTable - 1)]: FrameInput::table, or
                                             // the strided form (one base, no offsets)
    int width, height;
    long long row_stride, frame_stride;
    int tile_row_begin, tile_rows, tiles_x;
    int out_tile_rows;               // FrameInput::out_tile_rows
    int rgb_aligned8;                // every frame's base, row_stride and frame_stride are multiples of 8: whole tiles are read as 8-byte words
    const double* vec_in;
    int vec_channel;
    long long n_tc[3];               // tile-channels of each channel (tiles of the stripe x frames; vector mode: only vec_channel's is not 0)
    unsigned* queue;                 // [3] next tile-channel of each channel (zero before the launch)
    // per-wave scratch for the pairs (sizes: pursuit_scratch_*): a wave's own, whatever channel it works on
    float* pair_p;
    unsigned* pair_meta;
    float* pair_e;
    Outputs out;
    unsigned long long* stats;       // [2] += executed MFMA instructions, tile-channel-steps (one atomic per wave at exit); may be null
    unsigned long long* debug;       // diagnostic builds (-DMPC_STAMPS) only: 24 phase-cycle / event counters; else null
};

int launch_pursuit(const PursuitArgs& args, void* stream);       // grid = args.workgroups
size_t pursuit_scratch_floats(int workgroups);
size_t pursuit_scratch_meta(int workgroups);
size_t pursuit_scratch_bounds(int workgroups);
int pursuit_units_per_workgroup();
// Gram table of one channel (see mp_pursuit.hip); shadow[detail_rows]: 1 = row left out of the filter copy
int launch_gram(const double* base, const double* detail, const int32_t* block_rows, const int32_t* block_row_off,
                const uint8_t* shadow, float* gram, int num_base, int n_sel, long long stride, void* stream);
// The tests' probe of the screen (see mp_pursuit.hip): n <= 16 vectors of 64 doubles against the 32 tiles at base_tiles and the 4 at
// block_tiles; approx[n][576], bound[n].  vectors and approx 16-byte aligned.
int launch_screen_probe(const uint16_t* base_tiles, const uint16_t* block_tiles, const double* vectors, int n, float* approx, float* bound,
                        void* stream);
// The tests' probe of the key tracking (see mp_pursuit.hip): one wave; row_bits[64][144], pair_bits[64][16] (both 16-byte aligned),
// out[64][14].
int launch_track_probe(const unsigned* row_bits, const unsigned* pair_bits, float E, int rows, int pair, unsigned* out, void* stream);

// ---- device-side stream assembly (mp_streams.hip) ----
struct StreamArgs {
    const uint16_t* counts;          // [tiles][3]
    const uint32_t* choices;         // [tiles][3][K]
    long long tiles;
    int K;
    unsigned* block_live;            // [stream_workspace_words(tiles, K)] scratch
    unsigned* sizes;                 // [3][K] out: symbols per (channel, step)
    unsigned long long* stream_off;  // [6K + 1] out: stream boundaries in `symbols` (container order)
    uint16_t* symbols;               // [2 * 3 * K * tiles] worst case; out: the 6K streams back to back
    uint16_t* dc_tmp;                // [3][tiles] scratch
};
size_t stream_workspace_words(long long tiles, int K);
int launch_stream_assembly(const StreamArgs& a, void* stream);
// the decoder's way back: counts + the 6K streams (in `symbols`, container order, DC coefficients already summed) -> records
// [tiles][3][K], dead steps zero.  Uses a.counts, a.symbols (read), a.block_live and a.sizes (scratch); not a.stream_off / a.dc_tmp
int launch_stream_gather(const StreamArgs& a, uint32_t* choices, void* stream);

// ---- a pixel rectangle's share of the streams (mpc_decode_regions_indexed) ----
// The streams are compactions of the records in tile order, so the tiles [t0, t1) own the positions [r0, r1) of stream pair
// (channel, step): r = the tiles in front with more atoms than the step.  One WindowStream per stream of the 6K, on the device.
struct WindowStream {
    unsigned long long r0, r1;          // the window's expanded positions in the stream, r0 <= r1 <= the stream's size by the lengths
    unsigned c0, c1;                    // the chunks to parse, [r0 / interval, ceil(r1 / interval)) cut to the stream's chunks; a stream
                                        // that cannot be cut (run-length packed, a step-0 coefficient stream, "parse all"): all of them
};
// Index version 2: what a stream with aux entries (run-length packed, or a step-0 coefficient stream) is entered with at chunk c0
// and held to at chunk c1.  One per stream of the 6K, written by mp_window_rank_kernel<true>, every value cut to the host's sizes.
constexpr unsigned kSpanCut = 1u;       // WindowSpan::flags: the stream is cut by its aux entries (else: as without them)
constexpr unsigned kSpanCheck = 2u;     // ... c1 < n_chunks: the exit values are checkpoint c1's (else the stream's end: out1 = expect)
struct WindowSpan {
    unsigned long long s0, s1;          // the coded symbols parsed, [c0 * interval, min(c1 * interval, n_coded))
    unsigned long long out0, out1;      // the expansion's position in front of s0 and behind s1 - 1, out0 <= out1 <= expect
    unsigned state0, prev0, dc0;        // runLengthDecode's state at s0, coded symbol s0 - 1, the DC sum in front of out0
    unsigned state1, prev1, dc1;        // what must hold behind s1 - 1 (kSpanCheck)
    unsigned flags, reserved;
};
struct UnpackStream;
struct ParseStream;
struct WindowArgs {
    StreamArgs sa;                      // counts, tiles, K; block_live and sizes as the count and scan kernels leave them
    const UnpackStream* unpack;         // [6K]: which streams are packed
    const ParseStream* parse;           // [6K + 1]: every stream's chunks
    unsigned interval;
    int parse_all;                      // != 0: every stream whole
    long long t0, t1;                   // 0 <= t0 < t1 <= tiles
    WindowStream* window;               // out [6K]
    // index version 2 (span != null; launch_window_rank then runs mp_window_rank_kernel<true>), else unused
    const unsigned long long* aux;      // the aux entries as in the blob: (out, prev | dc << 16 | state << 32) each, checked by the host
    const unsigned long long* aux_off;  // [6K]: the stream's first entry (it has n_chunks of them), ~0 = it has none
    WindowSpan* span;                   // out [6K]
};
// count + scan over all tiles (cheap; every 1024-tile block's offset in every stream), then the ranks of t0 and t1
int launch_window_rank(const WindowArgs& w, void* stream);
// the gather for the blocks that hold the tiles [t0, t1) alone: other tiles' records are not written (nor their symbols read).
// a.block_live / a.sizes as launch_window_rank leaves them
int launch_stream_gather_window(const StreamArgs& a, uint32_t* choices, long long t0, long long t1, void* stream);
// quant[3 * K] (host memory, read before the call returns) -> dst[3 * K] on `stream`, as a kernel argument (mp_streams.hip)
struct QuantTable {
    double q[3 * kMaxDeviceK];
};
int launch_quant_table(const double* quant, int K, double* dst, void* stream);
// records of the tile rows [row_begin, row_begin + rows) in stripe order -> their places in the whole frame's records
int launch_interleave_stripe(const uint16_t* part_counts, const uint32_t* part_choices, int tiles_x, int tiles_y, int row_begin, int rows,
                             int K, uint16_t* frame_counts, uint32_t* frame_choices, void* stream);
// records of the tile grid [tx0, tx1) x [ty0, ty1) of a frame of tiles_x x tiles_y tiles -> the compact frame of that grid:
// out_counts[t' * 3 + ch] = min(count, steps, K), out_choices[(t' * 3 + ch) * K + i] = the record for i below that, else 0, with
// t' = (tx - tx0) * (ty1 - ty0) + (ty - ty0).  *error (the caller zeroes it) is set by a count above K in the grid.  steps >= 1
int launch_crop_records(const uint16_t* counts, const uint32_t* choices, int tiles_x, int tiles_y, int tx0, int ty0, int tx1, int ty1, int K,
                        int steps, uint16_t* out_counts, uint32_t* out_choices, int* error, void* stream);
// records of the grid of ncols x nty tiles at (stx0, sty0) of a frame of src_tiles_x x src_tiles_y tiles -> the grid of the same size at
// (dtx0, dty0) of a frame of dst_tiles_x x dst_tiles_y tiles, both in whole-frame layout: counts min(count, K), the records below that
// copied, the steps behind them zero.  owner: null, or per destination tile; then only tiles with owner[t] == part are written.
// *error (the caller zeroes it) is set by a count above K in a written tile
int launch_paste_records(const uint16_t* src_counts, const uint32_t* src_choices, int src_tiles_x, int src_tiles_y, int stx0, int sty0, int ncols,
                         int nty, int K, uint16_t* dst_counts, uint32_t* dst_choices, int dst_tiles_x, int dst_tiles_y, int dtx0, int dty0,
                         const int32_t* owner, int part, int* error, void* stream);
// mp_stream_scan_kernel alone: the exclusive scan over the blocks of the first `pairs` columns of a.block_live ([blocks][3 * a.K]),
// in place, each column's total in a.sizes[column].  Uses a.K, a.block_live and a.sizes only
int launch_stream_scan(const StreamArgs& a, int pairs, int blocks, void* stream);

// ---- the delta encoder's kernels (mp_delta.hip; include/mpcodec.h, "delta") ----
// Scratch of launch_tile_diff for a frame of `tiles` tiles: a flag per tile, then the 1024-tile blocks' counts.  One layout for the
// launch and for whoever allocates it.
size_t tile_diff_scratch_bytes(long long tiles);
// Tile t = tx * tiles_y + ty of the width x height frame at `rgb` (row_stride >= 3 * width, any alignment) against the tight copy `kept`
// (3 * width bytes a row): list[0 .. *count) = the tiles with a differing pixel byte, ascending; kept = the new pixels.  Only pixel
// bytes of `rgb` are read.  8-byte fetches when both bases, row_stride and 3 * width are multiples of 8, else byte by byte.
int launch_tile_diff(uint8_t* kept, const uint8_t* rgb, int width, int height, size_t row_stride, int32_t* list, int32_t* count, void* scratch,
                     void* stream);
// The same with a tolerance (host_delta.h: changed_tiles_tolerance): list = the tiles whose summed squared byte difference exceeds
// `tolerance`, and kept = the new pixels in those tiles only, its old ones in every other.  sse: NULL or [tiles], every tile's sum.
// totals: NULL or [2], zeroed on the stream first: the held tiles (0 < sum <= tolerance) and the sum of their sums.  Same scratch
int launch_tile_diff_tolerance(uint8_t* kept, const uint8_t* rgb, int width, int height, size_t row_stride, uint32_t tolerance, int32_t* list,
                               int32_t* count, uint32_t* sse, unsigned long long* totals, void* scratch, void* stream);
// The listed tiles of the frame as a packed frame of rows x cols whole tiles (host_delta.h: pack_geometry), listed tile j at
// (j / rows, j % rows); pixels outside the image, padding tiles and list entries outside [0, tiles) are black.  packed: 8-byte
// aligned, packed_stride a multiple of 8 and >= 24 * cols; bytes of a row behind 24 * cols are not written
int launch_tile_pack(const uint8_t* rgb, int width, int height, size_t row_stride, const int32_t* list, long long n, int rows, int cols,
                     uint8_t* packed, size_t packed_stride, void* stream);
// launch_tile_pack's inverse: the pixel bytes of listed tile j, at packed tile (j / rows, j % rows), to tile list[j] of the frame at
// `rgb` (row_stride >= 3 * width, any alignment), cut to the image; stride padding, the other tiles and the padding tiles' places are
// not written.  An entry outside [0, tiles) writes nothing and sets *error.  packed: 8-byte aligned, packed_stride a multiple of 8
// and >= 24 * cols.  8-byte stores when rgb and row_stride are multiples of 8 and the chunk lies whole in its row, else byte by byte
int launch_tile_unpack(const uint8_t* packed, size_t packed_stride, const int32_t* list, long long n, int rows, int cols, uint8_t* rgb, int width,
                       int height, size_t row_stride, int* error, void* stream);
// The packed frame's records j (3 counts, 3 * K words) to the whole-frame records at tile list[j]; an entry outside [0, tiles) is
// skipped and sets *error.  The entries are distinct
int launch_tile_scatter_records(const uint16_t* packed_counts, const uint32_t* packed_choices, const int32_t* list, long long n, int K,
                                uint16_t* counts, uint32_t* choices, long long tiles, int* error, void* stream);

// ---- rate control (mp_budget.hip; include/mpcodec.h, "budget") ----
// The depth profile: profile[t * (K + 1) + n] = the tile SSE launch_distortion gives for the same records with every count replaced
// by min(count, n), n = 0 ... K, for prefix-consistent records (a record's row lies in the dictionary its earlier steps built).  A
// record that is not, a row outside its dictionary and a count above K (used as K) set *error; no address comes from such a record
struct ProfileParams {
    const uint16_t* counts;          // [tiles][3], tile t = tx*tiles_y + ty
    const uint32_t* choices;         // [tiles][3][K]
    const double* quant;             // [3][K] (device), the values the container header carries
    int K;
    int width, height, tiles_x, tiles_y;
    const uint8_t* original;         // [height][width][3] (device)
    uint32_t* profile;               // [tiles][K + 1]
    int* error;
    int fast;                        // != 0: FromCoeffsDynamicFast (float)
};
int launch_depth_profile(const DictDevice& dict, const ProfileParams& p, void* stream);
// The allocation at one multiplier (host_budget.h: budget_allocate defines it): depth[tiles], out_counts[tiles][3], and
// totals[0 .. 2] += the distortion, the rate and the records kept (the caller zeroes them).  The weights travel in the kernel's arguments.
// emphasis != null: budget_allocate_emphasis, a code object of its own; null launches the plain kernel as before
struct AllocateParams {
    const uint32_t* profile;         // [tiles][K + 1]
    const uint16_t* counts;          // [tiles][3]
    long long tiles;
    int K;
    unsigned long long lambda;
    uint8_t* depth;
    uint16_t* out_counts;
    unsigned long long* totals;      // [3]
    uint32_t weights[3 * kMaxDeviceK];   // [3][K]
    const uint8_t* emphasis;         // [tiles] or null (host_budget.h, "emphasis")
};
int launch_budget_allocate(const AllocateParams& p, void* stream);
// The allocation's totals at all 256 multipliers in one launch (host_budget.h: budget_sweep defines it):
// totals[3 * j + 0 .. 2] += the distortion, the rate and the records kept at multiplier j (the caller zeroes the 768 words).
// At most kSweepGridCap workgroups whatever the frame, each adding 768 totals once.  The weights travel in the kernel's arguments
constexpr int kSweepGridCap = 512;
constexpr int kSweepTiles = 16;          // tiles a workgroup stages at a time
struct SweepParams {
    const uint32_t* profile;         // [tiles][K + 1]
    const uint16_t* counts;          // [tiles][3]
    long long tiles;
    int K;
    unsigned long long* totals;      // [256][3]
    uint32_t weights[3 * kMaxDeviceK];   // [3][K]
    const uint8_t* emphasis;         // [tiles] or null: budget_sweep_emphasis, as for AllocateParams
};
// host_budget.h: emphasis_from_mask.  mask[height][row_stride] (device, any alignment) -> emphasis[tiles_x * tiles_y], x-outer / y-inner
int launch_emphasis_mask(const uint8_t* mask, int width, int height, size_t row_stride, int lo, int hi, uint8_t* emphasis, void* stream);
int launch_budget_sweep(const SweepParams& p, void* stream);
// The two for a group of frames of one geometry (host_budget.h: budget_allocate_group, budget_sweep_group define them): tile t of frame f
// is tile f * tiles + t of every array.  A launch takes up to kGroupChunk frames, the frame as blockIdx.y, their weights in the
// kernel's arguments at weights[f * 3 * kMaxDeviceK + ch * K + i]; the launchers below cut a group into such launches, one behind the
// other on `stream`.  weights: host memory, [frames][3][K], read before the launcher returns.  totals: the allocation's
// [frames][3], the sweep's [256][3] summed over the frames; the caller zeroes them.  emphasis: [frames * tiles] or null
constexpr int kGroupChunk = 8;
struct AllocateGroupParams {
    const uint32_t* profile;         // [frames][tiles][K + 1]
    const uint16_t* counts;          // [frames][tiles][3]
    long long tiles;                 // of one frame
    int K, frames;                   // frames of this launch, 1 ... kGroupChunk
    unsigned long long lambda;
    uint8_t* depth;
    uint16_t* out_counts;
    unsigned long long* totals;      // [frames][3]
    const uint8_t* emphasis;
    uint32_t weights[kGroupChunk * 3 * kMaxDeviceK];
};
struct SweepGroupParams {
    const uint32_t* profile;
    const uint16_t* counts;
    long long tiles;
    int K, frames;
    unsigned long long* totals;      // [256][3]
    const uint8_t* emphasis;
    uint32_t weights[kGroupChunk * 3 * kMaxDeviceK];
};
int launch_budget_allocate_group(const uint32_t* profile, const uint16_t* counts, const uint8_t* emphasis, int frames, long long tiles, int K,
                                 const uint32_t* weights, unsigned long long lambda, uint8_t* depth, uint16_t* out_counts,
                                 unsigned long long* totals, void* stream);
int launch_budget_sweep_group(const uint32_t* profile, const uint16_t* counts, const uint8_t* emphasis, int frames, long long tiles, int K,
                              const uint32_t* weights, unsigned long long* totals, void* stream);

// ---- a delta stream to a byte budget (mp_rate.hip; include/mpcodec.h, "rate") ----
// The tail of launch_tile_diff alone (mp_delta.hip): list[0 .. *count) = the tiles whose flag byte is not 0, ascending.  block_live:
// 3 words per 1024 tiles, as tile_diff_scratch_bytes lays them out behind the flags
int launch_tile_flags_list(const uint8_t* flags, long long tiles, unsigned* block_live, int32_t* list, int32_t* count, void* stream);
unsigned* tile_diff_block_live(void* scratch, long long tiles);
// host_rate.h: owed_tiles, per tile.  flags[t] != 0 on entry: tile t is changed; on return flags[t] != 0: tile t is a candidate
// (bit 1 = owed: sent[t] < max over ch of min(counts[t * 3 + ch], K)).  must[t] = changed, floor[t] = changed ? 0 : sent[t]
int launch_owed_flags(const uint8_t* sent, const uint16_t* counts, long long tiles, int K, uint8_t* flags, uint8_t* floor, uint8_t* must,
                      void* stream);
// The scatter turned round, with a cut: packed tile j < n takes the records of candidate c = idx ? idx[j] : j, tile list[c], with the
// counts min(count, K, depth ? depth[c] : K); every entry at or above that count is 0, and so are the counts and entries of the padding
// tiles n <= j < padded.  c outside [0, m) or list[c] outside [0, tiles): that packed tile is all 0 and *error is set
struct GatherParams {
    const uint16_t* counts;          // [tiles][3]
    const uint32_t* choices;         // [tiles][3][K]
    long long tiles;
    const int32_t* list;             // [m]
    long long m;
    const int32_t* idx;              // [n] or null
    const uint8_t* depth;            // [m] or null
    long long n, padded;
    int K;
    uint16_t* out_counts;            // [padded][3]
    uint32_t* out_choices;           // [padded][3][K]
    int* error;
    const uint8_t* tile_bytes[2];    // each null, or a byte per tile that travels with the records (a call's floor and must) ...
    uint8_t* out_bytes[2];           // ... to [padded]; 0 for a padding tile
};
int launch_gather_records(const GatherParams& p, void* stream);
// A budget call's commit: sent[list[c]] = depth ? depth[c] : K for c = idx ? idx[j] : j, j < n; entries outside their ranges are skipped
int launch_sent_commit(const int32_t* list, long long m, const int32_t* idx, const uint8_t* depth, long long n, int K, uint8_t* sent,
                       long long tiles, void* stream);
// The allocation with a floor at one multiplier (host_rate.h: budget_allocate_floor defines it): depth[n], out_counts[n][3], send[n],
// totals[0 .. 3] += (the caller zeroes them).  floor, must: null = all 0, all 1
struct AllocateFloorParams {
    const uint32_t* profile;         // [n][K + 1]
    const uint16_t* counts;          // [n][3]
    const uint8_t* floor;            // [n] or null
    const uint8_t* must;             // [n] or null
    long long n;
    int K;
    unsigned long long lambda;
    uint8_t* depth;
    uint16_t* out_counts;
    uint8_t* send;
    unsigned long long* totals;      // [4]
    uint32_t weights[3 * kMaxDeviceK];   // [3][K]
    const uint8_t* emphasis;         // [tiles] or null: budget_allocate_floor_emphasis, candidate i takes emphasis[list ? list[i] : i] ...
    const int32_t* list;             // [n] or null
    long long tiles;                 // ... and the neutral value where that tile is outside [0, tiles)
};
int launch_budget_allocate_floor(const AllocateFloorParams& p, void* stream);

// ---- the decoder's per-symbol work in front of the gather (mp_unpack.hip): run-length expansion, DC sums ----
constexpr int kUnpackBlock = 2048;      // coded symbols per workgroup
constexpr unsigned kUnpackPacked = 1u;  // UnpackStream::flags: the stream is run-length packed

struct UnpackStream {                   // one per stream, built by the host from sizes it has checked; [n_streams] is a sentinel
    unsigned long long coded_off;       // first symbol of the stream in `coded`
    unsigned long long coded_len;       // its symbols as entropy-decoded
    unsigned long long expect;          // symbols it must expand to (from the lengths stream)
    unsigned long long out_off;         // its first symbol in `symbols`: the sum of `expect` of the streams in front of it
    unsigned blk_begin;                 // its first block; it has ceil(coded_len / kUnpackBlock) of them.  Sentinel: n_blocks
    unsigned flags;
};

struct UnpackArgs {
    const uint16_t* coded;              // the streams as entropy-decoded, back to back; an even number of symbols is allocated
    const UnpackStream* streams;        // [n_streams + 1]
    int n_streams;                      // 6K
    unsigned n_blocks;
    unsigned* blk_piece;                // [n_blocks][4] scratch, 16-byte aligned: state map and symbols emitted per entry state
    unsigned* blk_entry;                // [n_blocks] scratch: the state a block is entered in
    unsigned long long* blk_out;        // [n_blocks] scratch: the block's first output position in its stream
    unsigned* stream_ok;                // [n_streams] scratch: the stream expands to exactly `expect` symbols
    uint16_t* symbols;                  // out: sum(expect) symbols (an even number allocated), the layout launch_stream_gather reads
    int* error;                         // |= 1 when a stream does not expand to `expect` symbols; nothing is written for that stream
    int dc_stream[3];                   // the step-0 coefficient streams: 1, 2K + 1, 4K + 1
    unsigned dc_blk_begin[4];           // their blocks of kUnpackBlock expanded symbols: prefix sums of ceil(expect / kUnpackBlock)
    unsigned* dc_part;                  // [dc_blk_begin[3]] scratch: each block's sum of differences
    const WindowStream* window;         // launch_unpack_window alone: [n_streams], on the device
};
int launch_unpack(const UnpackArgs& a, void* stream);                // hipError_t as int
// the same with the copy of a stream that is neither packed nor a step-0 coefficient stream limited to the blocks that hold its
// window [r0, r1); packed streams and the DC sums as in launch_unpack
int launch_unpack_window(const UnpackArgs& a, void* stream);
// Index version 2: launch_unpack_window where, besides, a stream with kSpanCut is expanded (and summed) from its entry values over
// the coded symbols [s0, s1) alone and held to its exit values before anything of it is written; a.window and span on the device
struct UnpackWindowArgs {
    UnpackArgs a;
    const WindowSpan* span;             // [n_streams]
};
int launch_unpack_window_cut(const UnpackWindowArgs& w, void* stream);

// ---- the entropy codes of a container parsed on the device, chunk by chunk from a seek index (mp_parse.hip) ----
constexpr int kParseLutBits = 11;       // the Huffman window, HuffmanCodebook::kLutBits
constexpr int kParseGroup = 64;         // chunks a wave decodes, one a lane: consecutive chunks of one stream
constexpr unsigned kParseGolomb = 1u;   // ParseStream::flags
constexpr unsigned kParseLengths = 2u;  // the lengths stream: its symbols go to `counts`, cut to K
constexpr unsigned kParseLutEof = 1u << 24;

struct ParseStream {                    // one per stream (the lengths stream first), built by the host from an index it has checked
    unsigned long long out_off;         // its first symbol in `coded` (UnpackStream::coded_off); the lengths stream: 0, in `counts`
    unsigned long long n_coded;         // symbols its codes yield
    unsigned long long end_bit;         // the bit behind the stream (behind the pseudo-EOF for Huffman), <= 8 * the container's bytes
    unsigned long long cp_off;          // its first checkpoint in `checkpoints`; it has n_chunks of them
    unsigned long long expect;          // symbols it must expand to, as the index says: checked against the decoded lengths
    unsigned n_chunks;                  // ceil(n_coded / interval)
    unsigned group_begin;               // its first group of kParseGroup chunks.  Sentinel [n_streams]: n_groups
    unsigned flags;
    unsigned m;                         // Golomb parameter (>= 1)
    unsigned lut_off;                   // Huffman: its window table in `luts`, 1 << kParseLutBits entries:
                                        //   symbol | length << 16 | kParseLutEof for the pseudo-EOF; 0 = no code this short
    unsigned len_off;                   // ... its per-length table in `lens`: [33][3] = codes of length l, first code, first entry
    unsigned table_off;                 // ... its entry -> symbol table in `tables`, `total` entries
    unsigned total;                     // ... entries; total - 1 is the pseudo-EOF
    unsigned max_length;                // ... <= 32
    unsigned reserved;
};

struct ParseArgs {
    const uint32_t* words;              // the container's bytes, zero-padded to a whole word and 16 bytes beyond
    const unsigned long long* checkpoints;
    const ParseStream* streams;         // [n_streams + 1]
    const uint32_t* luts;
    const uint32_t* lens;
    const uint16_t* tables;
    int n_streams;                      // 6K + 1
    int K;
    unsigned interval;
    unsigned n_groups;
    unsigned long long n_counts;        // 3 * tiles
    uint16_t* coded;                    // out: UnpackArgs::coded
    uint16_t* counts;                   // out: the lengths, every one <= K (an even number of symbols allocated, as for `coded`)
    unsigned* hist;                     // [3][kMaxDeviceK + 1] + 1 scratch: the lengths' histogram per channel; [last]: sizes differ
    int* error;                         // |= 1: a chunk did not decode to exactly its symbols and its end, a length above K,
                                        // or stream sizes other than the index says
    const WindowStream* window;         // launch_parse_window alone: [n_streams - 1], on the device, for streams 1 .. 6K
    unsigned group_first;               // ... the first group of its grid: streams[1].group_begin
};
int launch_parse(const ParseArgs& a, void* stream);                  // hipError_t as int
// launch_parse in two halves for a frame of which a window is wanted: the lengths stream's groups with hist / verify / void, and --
// once launch_window_rank has written a.window -- the 6K streams' groups, of which only the chunks [c0, c1) of each stream are read
int launch_parse_lengths(const ParseArgs& a, void* stream);
int launch_parse_window(const ParseArgs& a, void* stream);
// A view of the first `steps` steps: a.counts cut in place to min(count, steps), behind launch_parse_lengths -- whose verify kernel
// has compared the UNCUT sizes with the index's -- and in front of launch_window_rank, whose count and scan then give a stream of a
// step at or above `steps` size 0 and the ranks (0, 0), and of the gather, which lays the streams out by these lengths.  The host's
// UnpackStream / ParseStream tables hold those streams empty (no chunks, no symbols), so both layouts agree
int launch_clamp_lengths(const ParseArgs& a, int steps, void* stream);

// ---- the seek index's checkpoints from a bit scan (mp_scan.hip; the host form is HostStreamScanner, host_container.cpp) ----
// One window of one stream: bits [win_begin, win_begin + win_bits) of the container, win_begin a code start of the stream with
// ordinal `ord0` (the stream's first code bit, or the position the window before carried over).  All positions below are relative
// to win_begin and fit 30 bits: win_bits <= 2^26, a code takes at most kScanUnaryCap + 34 bits.
constexpr unsigned kScanUnaryCap = 1u << 16;        // a Golomb unary run this long is no code to the scan (host_bitstream.h: kScanUnaryLimit)
constexpr unsigned kScanSuper = 64;                 // segments a super-segment holds
// a step: the code's bits in the low 24 | the pseudo-EOF | no code here (or it would pass the container's end)
constexpr unsigned kScanStepDead = 0x80000000u, kScanStepEof = 0x40000000u, kScanStepLen = 0x00FFFFFFu;
// an exit: a code start at or behind the segment's (super-segment's) end | the bit behind the pseudo-EOF | the path dies
constexpr unsigned kScanExitDead = 0x80000000u, kScanExitEof = 0x40000000u, kScanExitPos = 0x3FFFFFFFu;
constexpr unsigned kScanNoEntry = 0xFFFFFFFFu;
// ScanResult::state
constexpr unsigned kScanContinue = 1u, kScanEnded = 2u, kScanDead = 3u, kScanMiscount = 4u;
struct ScanResult {
    unsigned state;                     // 0 = nothing written (a defect); continue: the stream goes on behind the window at
    unsigned final_seg;                 //   `position` with ordinal `ordinal`; ended: `position` is the bit behind the stream and
    unsigned long long position;        //   `ordinal` its codes; dead / miscount: the scan gives up
    unsigned long long ordinal;
};
struct ScanArgs {
    ParseArgs tables;                   // words (the container, zero-padded as for the parse), luts, lens, tables: this stream's own
    ParseStream stream;                 // flags (Golomb), m, lut_off / len_off / table_off (0), total, max_length
    unsigned long long total_bits;      // 8 * the container's bytes: every step's required end
    unsigned long long win_begin;       // < total_bits
    unsigned long long ord0;
    unsigned long long n;               // the codes the stream must hold
    unsigned win_bits;                  // <= total_bits - win_begin
    unsigned seg_bits;                  // 32 ... 32768
    unsigned n_segs;                    // ceil(win_bits / seg_bits)
    unsigned n_supers;                  // ceil(n_segs / kScanSuper)
    unsigned interval;
    unsigned long long n_cp;            // ceil(n / interval): the stream's share of `checkpoints`
    unsigned* step;                     // [win_bits]
    unsigned* exit_of;                  // [win_bits]
    uint16_t* count;                    // [win_bits] codes on the path to the exit (<= seg_bits)
    unsigned* sup_exit;                 // [n_supers * seg_bits]: from the bits of a super-segment's first segment, over its segments
    unsigned* sup_count;                // [n_supers * seg_bits]
    unsigned* sup_entry;                // [n_supers] the chain's entry (kScanNoEntry: it jumped no such super-segment whole)
    unsigned long long* sup_ord;        // [n_supers]
    unsigned* seg_entry;                // [n_segs] the chain's entry into each segment (kScanNoEntry: none)
    unsigned long long* seg_ord;        // [n_segs] the ordinal of the code at that entry
    unsigned long long* checkpoints;    // [n_cp] out: the container bit of code j * interval
    ScanResult* result;                 // out
};
// step table, segment maps, super-segment maps, chain, emit: five launches on `stream`.  hipError_t as int
int launch_scan_window(const ScanArgs& a, void* stream);

// ---- device-side entropy stage (mp_entropy.hip): everything that touches every symbol of the 1 + 6K streams ----
constexpr int kEntBlock = 4096;         // symbols per scan block
constexpr int kEntHistSpan = 4;         // scan blocks per histogram span and range of symbol values (ent_hist_kernel)
constexpr int kEntMaxStreams = 6 * kMaxDeviceK + 1;

struct EntStream {                      // one per stream; the device fills the first part, the host the second
    unsigned long long raw_off;         // first symbol of the stream in `symbols` (stream 0 = `lengths`: the counts array)
    unsigned n;                         // symbols of the stream as assembled
    unsigned blk_begin;                 // first scan block
    unsigned rle_size;                  // symbols runLengthEncode emits (Huffman.cpp:246-279)
    unsigned shorter;                   // 1 = the run-length coded stream is what gets coded (CompressedImage.cpp:450)
    unsigned eff_n;                     // symbols that get coded
    unsigned largest;                   // largest of them
    unsigned distinct, triple_off;      // its (symbol, count, first position) triples in `triples`
    unsigned mode;                      // host: 0 = Huffman (dense table), 1 = Golomb
    unsigned m;                         // host: Golomb parameter
    unsigned reserved;                  // phase 1: the compaction's write cursor.  Phase 2, host: its first slot in `checkpoints`
    unsigned long long bit_off;         // host: bit offset of the stream's first code in the container
    unsigned long long coded_bits;      // device: bits written for the stream's symbols
};

struct EntropyArgs {
    const uint16_t* counts;             // [n_lengths] the lengths stream
    const uint16_t* symbols;            // the 6K code streams back to back (StreamArgs::symbols)
    const unsigned long long* stream_off;   // [6K + 1]
    unsigned n_lengths;
    int n_streams;                      // 6K + 1
    uint16_t* packed;                   // run-length coded streams, at the offsets of their sources (capacity of `symbols`)
    EntStream* streams;                 // [n_streams]
    unsigned* totals;                   // [4]: scan blocks, (unused), triples written, triple overflow flag
    unsigned* blk_stream;               // per scan block: the stream it belongs to
    unsigned* blk_lead;                 // per scan block: symbols in front of its first run start | run ends there << 31
    unsigned* blk_inner;                // ... run-length symbols emitted for the runs that start inside the block
    unsigned* blk_tail;                 // ... symbols from its last run start to its end
    unsigned* blk_carry;                // ... symbols of the run its first symbol continues, in front of the block
    unsigned* blk_out;                  // ... first run-length symbol of the block in the packed stream
    unsigned* blk_bits;                 // ... code bits
    unsigned long long* blk_bit_off;    // ... bit offset of its first code in the container
    unsigned* ghist;                    // [n_streams][65536] zero between calls
    unsigned* gfirst;                   // [n_streams][65536] 0xFFFFFFFF between calls
    unsigned* triples;                  // [triple_cap][3], in (mapped) host memory: the compaction writes it across PCIe
    unsigned triple_cap;
    EntStream* host_streams;            // [n_streams] mirror of `streams` in (mapped) host memory
    unsigned* host_totals;              // [4] mirror of `totals`
    unsigned* tcode;                    // [n_streams][65536] zero between calls
    uint8_t* tlen;                      // [n_streams][65536]
    const unsigned* entries;            // [n_entries][3]: stream << 16 | symbol, code, length (may be mapped host memory)
    unsigned n_entries;
    unsigned cp_interval;               // seek index: coded symbols per checkpoint, 32 ... 65536 (read only where `checkpoints` is set)
    unsigned* out32;                    // the container, zeroed
    unsigned long long out_words;
    // seek index (null: none): the container bit of coded symbol c * cp_interval of stream s at [streams[s].reserved + c], stream
    // behind stream -- the index blob's own layout.  cp_capacity entries; nothing is written beyond them
    unsigned long long* checkpoints;
    unsigned cp_capacity;
    // seek index version 2 (null: none; phase 1 reads cp_interval with it): the aux entries of the streams that are packed or step-0
    // coefficient streams, two words each -- out, then prev | dc << 16 | state << 32 -- entry c of stream s at [aux_first[s] + c],
    // stream behind stream and only those streams: the blob's aux section.  aux_capacity entries; nothing is written beyond them
    unsigned long long* aux;
    unsigned aux_capacity;
    unsigned* aux_first;                // [n_streams] device: entries of the streams in front (ent_aux_offsets_kernel)
    unsigned* blk_dc;                   // per scan block of a step-0 coefficient stream: wrapping sum of zigzagDecode over its raw symbols
};
size_t entropy_max_blocks(unsigned long long symbols, int n_streams);
// checkpoints the streams of a frame can have at most, whatever the interval (>= 32): sum of ceil(eff_n / interval)
size_t entropy_max_checkpoints(unsigned long long capacity_symbols, int n_streams);
// capacity_symbols: upper bound of the symbols in all streams (lengths included); hipError_t as int.  With a.aux set the pack pass
// also records the aux entries' out, prev and state and two more kernels add the step-0 streams' sums; otherwise the launches are
// exactly those of a call without
int launch_entropy_phase1(const EntropyArgs& a, unsigned long long capacity_symbols, void* stream);
// raw_symbols: symbols in all streams as assembled (sum of EntStream::n).  With a.checkpoints set the code-writing pass also
// records the seek index's checkpoints; otherwise the launches are exactly those of a call without an index
int launch_entropy_phase2(const EntropyArgs& a, unsigned long long raw_symbols, void* stream);

// bytes of workspace needed for `cap` tile-channels and K steps
size_t workspace_bytes(int cap, int K);
// carve a workspace out of one device allocation of workspace_bytes(cap, K) bytes
Workspace carve_workspace(void* device_mem, int cap, int K);

}  // namespace mpc
