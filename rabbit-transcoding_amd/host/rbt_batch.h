// Host orchestration of one call: a "batch" is every picture of the sub-bitstreams handed over together (one GOF's
// geometry + attribute + occupancy streams in rbt_transcode_gof, a single stream in rbt_transcode_substream).
// The host parses NAL units, parameter sets and slice headers, lays the batch out in one HBM arena, uploads the
// unescaped slice data once, and enqueues the kernels; pictures never leave HBM between decode and re-encode.
#pragma once
#include <string>
#include <vector>
#include "../../include/rbt.h"
#include "../csrc/rbt_kernels.h"
#include "../csrc/rbt_hash.h"
#include "../csrc/rbt_rate.h"
#include "../csrc/rbt_quality.h"
#include "../csrc/rbt_ctbsse.h"
#include "rbt_hls.h"

namespace rbt {

struct StreamIn { const uint8_t* p; size_t n; };
struct FrameInfo { int stream; int nal_type; int hash_kind; uint8_t hash[48]; bool sao; uint64_t vcl_bytes; };   // hash_kind: RBT_HASH_* of the picture's hash SEI (0: none), hash: parse_hash_sei;
// vcl_bytes: the picture's VCL NAL units as they stand in the input (start codes excluded, emulation prevention bytes included): B_k of the rate estimate

// Decoded picture hashes of pictures in device memory (csrc/rbt_hash.h). add() the pictures, upload() before the first kernel of the stream
// (one copy: the picture table, the per-class lists and the zeroed state, results and counters), launch() behind the kernels that make the
// pictures, fetch() once the stream has got there: 48 bytes per picture and one mismatch count per counter come back.
struct HashSet {
  std::vector<RbtHashPic> pics; int n_counters = 0;
  std::vector<uint8_t> staging;                  // the upload, alive until it has completed
  uint8_t* d = nullptr; size_t o_lists = 0, o_state = 0, o_out = 0, o_end = 0;
  int n_class[6] = {}, class_off[6] = {}, class_luma[6] = {}, class_h[6] = {};   // class = (kind - 1) * 2 + (bit depth > 8)
  std::vector<uint8_t> out; std::vector<uint32_t> counters;
  int add(const uint16_t* const planes[3], int w, int h, int bit_depth, int kind, int counter = -1, const uint8_t* want = nullptr);   // index of the picture, < 0: refused
  bool empty() const { return pics.empty(); }
  int upload();
  void launch() const;
  int fetch();
  ~HashSet() { rbtk::dev_free(d); }
};

// Level census of decoded pictures in device memory (csrc/rbt_rate.h), used like HashSet: add() the pictures, upload() before the first kernel of the stream (one copy: the
// picture table and the zeroed histograms), launch() behind the kernels that leave the levels and the per-unit QPs (and before an encoder that shares the decoder's arena
// writes there), fetch() once the stream has got there: RBT_RATE_HIST_WORDS words per picture come back.
struct CensusSet {
  std::vector<RbtCensusPic> pics; int max_words = 0;
  std::vector<uint8_t> staging; uint8_t* d = nullptr; size_t o_hist = 0;
  std::vector<uint32_t> hist;                    // after fetch(): hist[3][53] per picture, in add() order
  int add(const RbtFrame& f);                    // index of the picture, < 0: refused (size not a multiple of 8)
  bool empty() const { return pics.empty(); }
  int upload();
  void launch() const;                           // between the events of T_CENSUS on the current stream
  int fetch();
  ~CensusSet() { rbtk::dev_free(d); }
};

// Distortion sums of picture pairs in device memory (csrc/rbt_quality.h), used like CensusSet: add() the pairs, upload() before the first kernel of the stream (one copy: the
// pair table and the zeroed sums), launch() behind the encoder's last filter, fetch() once the stream has got there: RBT_SSE_WORDS 64-bit words per pair come back.
// With `ext` set before upload() the sums live there instead (RBT_SSE_WORDS words per pair, zeroed by the owner): an encode batch keeps them behind its slice table, and
// they come back with the slice sizes in one copy (encode_finish).
struct SseSet {
  std::vector<RbtSsePic> pics; int max_chunks = 0; uint64_t* ext = nullptr;
  std::vector<uint8_t> staging; uint8_t* d = nullptr; size_t o_out = 0;
  std::vector<uint64_t> words;                   // after fetch(): {sse, sse_occ, n_occ} x 3 planes per pair, in add() order
  void add(const RbtSsePic& p);
  bool empty() const { return pics.empty(); }
  int upload();
  void launch() const;
  int fetch();
  ~SseSet() { rbtk::dev_free(d); }
};

enum { T_PARSE = 0, T_RECON = 1, T_CENSUS = 2, T_ANALYSE = 3, T_ENCODE = 4, T_ENTROPY = 5, T_ALL = 6, T_POOL = 7, T_INTER = 8, T_ENTROPY_I = 9, T_COUNT = 10 };   // (the device keeps 16 events per lane, rbt_pcc.cpp has the other six; T_CENSUS took the slot of a filter timer nothing used)

// Bump allocator over one device allocation, every buffer on a multiple of 256 bytes. A batch names each buffer of its arena once, in a layout function (decode_lay_out,
// encode_lay_out) that runs twice: without a base it only counts (take() gives nullptr, `used` ends as the size), over the allocated block it hands out the pointers.
struct Arena {
  uint8_t* base = nullptr; size_t used = 0;
  size_t mark() { return used = (used + 255) & ~(size_t)255; }          // where the next buffer will start
  template <class T> T* take(size_t count) { const size_t o = mark(); used = o + count * sizeof(T); return base ? (T*)(base + o) : nullptr; }
  // the three planes of a 4:2:0 picture (ys luma, cs chroma samples each) are one buffer: a new one, or one that exists elsewhere
  template <class T> void take_planes(T* p[3], size_t ys, size_t cs) { same_planes(p, take<T>(ys + 2 * cs), ys, cs); }
  template <class T> static void same_planes(T* p[3], T* first, size_t ys, size_t cs) { p[0] = first; p[1] = first ? first + ys : nullptr; p[2] = first ? first + ys + cs : nullptr; }
  static uint8_t* up256(uint8_t* p) { return (uint8_t*)(((uintptr_t)p + 255) & ~(uintptr_t)255); }
};
// One reconstruction launch of a dependency level (launch_recon). recon_level_of fills the counts; whoever owns the memory binds the pointers (decode_lay_out for a batch's
// own levels, launch_merged in rbt_transcode.cpp for levels merged across batches).
struct DecodeBatch;
struct LevelPic { const DecodeBatch* b; int frame; };
struct ReconLevel {
  RbtFrame* frames = nullptr; const RbtSlice* slices = nullptr; const int32_t* list = nullptr;   // the pictures as a frame list of one batch (an own level), nullptr for a merged level
  const RbtFrameRef* refs = nullptr; int n = 0, w_ctb = 0, h_ctb = 0;                           // ... as RbtFrameRef; their number; the largest picture
  uint32_t ctbs = 0; int queue_wgs = 0; uint32_t* queue = nullptr; uint32_t* ticket = nullptr;   // ready queue: CTBs of all pictures, workgroups, recon_queue_words(ctbs) zeroed words; flag form: a zeroed word
};
// DecodeBatch::d_tickets, zeroed words: flag launch of the batch's own level l / of merged level l (in the lead batch), ordered hand-out of the parse tasks of level l / of a merged parse launch
enum { TICKET_OWN_LEVEL = 0, TICKET_MERGED_LEVEL = 32, TICKET_PARSE = 64, TICKET_MERGED_PARSE = 96, TICKET_WORDS = 128, MAX_LEVELS = 32 };

struct DecodeBatch {
  std::vector<uint8_t> rbsp;
  std::vector<RbtFrame> frames; std::vector<RbtSlice> slices; std::vector<FrameInfo> info;
  std::vector<int> stream_first, stream_count;
  std::vector<Sps> stream_sps; std::vector<Pps> stream_pps;
  std::vector<std::vector<int>> level_frames;
  bool ordered_parse = false, lists_uploaded = false;
  std::vector<char> alias_taken;       // per stream: its pictures' dead buffers (coefficient levels, pre-SAO samples) have been handed to an encoder stream (setup_encode)
  bool recon_external = false;         // ... and reconstructed by merged per-level launches (launch_recon_refs + decode_launch_filters)
  bool parse_external = false;         // the batch's slices are parsed by a merged launch of the caller (launch_parse_tasks)
  std::vector<int32_t> lists_keep;     // host staging of the index lists, alive until the copy has completed
  std::vector<size_t> fr_off;          // offset of each level's frame list inside d_lists
  std::vector<size_t> sl_off, sl_cnt;  // slice list of each level inside d_lists
  std::vector<uint32_t> order_keep; std::vector<size_t> order_off;   // CTB dependency order per picture (host staging, offset per frame)
  std::vector<RbtFrameRef> refs_keep;   // the pictures of every level as RbtFrameRef, level by level (host staging)
  std::vector<ReconLevel> levels;       // the reconstruction launch of each level
  bool has_row_tasks = false;      // some segment of a wavefront stream is parsed by a wave of its own (ordered hand-out of the parse tasks, no banded parsing)
  uint32_t* d_order = nullptr; RbtFrameRef* d_refs = nullptr; uint32_t* d_tickets = nullptr;   // d_tickets: TICKET_WORDS counters (TICKET_* above)
  void* d_save = nullptr;              // RbtParseSave per slice (resumable parsing), zero-initialised; nullptr when not requested
  bool want_save = false;              // set before decode_build to reserve d_save
  void* arena = nullptr; size_t arena_size = 0;
  RbtFrame* d_frames = nullptr; RbtSlice* d_slices = nullptr; uint8_t* d_rbsp = nullptr; int32_t* d_lists = nullptr;
  CensusSet census; std::vector<int> census_first;   // rate targets: the pictures of the streams that are counted (census_first[stream]: index of the stream's first picture in `census`, -1: not counted)
  HashSet hash; std::vector<int> hash_checked;   // verify_md5: the pictures of the checked streams (counter = stream), pictures checked per stream
  int n_flat = 0;                      // after decode_finish: pictures reconstructed with flat chroma (RbtFrame::chroma_flat, read back with the error words)
  std::string err; int err_code = 0;
  ~DecodeBatch() { rbtk::dev_free(arena); }
};

int decode_build(DecodeBatch& b, const StreamIn* streams, int n);
int recon_mode();                    // 0 = one launch per anti-diagonal, 1 = one launch per level with neighbour flags, 2 = one launch per level with a ready queue (rbt_decode.cpp)
ReconLevel recon_level_of(const std::vector<LevelPic>& pics, std::vector<RbtFrameRef>* refs = nullptr);   // counts of the level made of `pics`; with `refs`, the pictures are appended there (their batches must be laid out)
int recon_mode_for(const ReconLevel* lv, size_t n);   // recon_mode() for these levels: by diagonals if one of them is too large for the ready queue's 31-bit entries
void launch_recon(const ReconLevel& lv, int mode);   // the only caller of the level-wide reconstruction launches of rbt_kernels.h
void recon_set_depth(int depth);     // jobs the caller keeps in flight (rbt_set_depth)
int decode_launch(DecodeBatch& b);   // enqueue every decode kernel of the batch on the current stream (no wait)
int decode_launch_parse(DecodeBatch& b);            // index lists + entropy decoding
int decode_upload_lists(DecodeBatch& b);            // index lists only (first half of decode_launch_parse)
int decode_max_w4(const DecodeBatch& b);            // width of the widest picture in 4-sample units
// Entropy decoding in `chunks` row bands with the reconstruction of each finished band of the level-0 pictures enqueued on
// stream `aux` underneath the parsing of the next band; ends with level 0 complete (filters included) on the current stream.
int decode_launch_chunked(DecodeBatch& b, int chunks, int main_stream, int aux_stream);
void decode_launch_level(DecodeBatch& b, size_t l);  // reconstruction + loop filters of dependency level l
void decode_launch_filters(DecodeBatch& b, size_t l); // loop filters of level l only
int decode_finish(DecodeBatch& b);   // wait for the batch's stream and check the per-picture error words
int decode_run(DecodeBatch& b);      // launch + finish
// verify_md5: every picture of the streams with verify[stream] that carries a hash SEI goes into b.hash (uploaded on the current stream); decode_launch_hash
// enqueues the hashing behind the decoder's last filter, decode_hash_result reads what came back (after hash.fetch()) for one stream
int decode_hash_setup(DecodeBatch& b, const std::vector<char>& verify);
void decode_launch_hash(const DecodeBatch& b);
void decode_hash_result(const DecodeBatch& b, int stream, int& checked, int& failed);
// rate targets: every picture of the streams with want[stream] goes into b.census (uploaded on the current stream); b.census.launch() goes behind the decoder's last filter
int decode_census_setup(DecodeBatch& b, const std::vector<char>& want);
int decode_fetch(DecodeBatch& b, int stream, rbt_video* out);   // the stream's cropped pictures to the host

size_t frame_samples(const RbtStreamCfg& c);

}  // namespace rbt
