// Launchers of the device kernels (one translation unit per kernel family: gen.hip, lattice.hip, fused.hip, pack.hip, wakati.hip, mecab.hip, detail.hip, format.hip, split.hip), as plain
// functions the host side (engine.hip: Tokenizer, Workspace) calls.  Every launcher enqueues on `stream` and returns.
#pragma once
#include <hip/hip_runtime.h>

#include "engine.hpp"
#include "format.hpp"

namespace vbt {

// Compact connector (Raw / Dual) as expand_connector reads it (pack.hip); all pointers are device pointers.
struct DevConnector {
    const uint32_t* bases; const uint32_t* checks; const int32_t* costs;
    uint32_t n_bases, n_checks;
    const uint32_t* right_feats; const uint32_t* left_feats;
    uint32_t width;
    const int16_t* m; const uint16_t* right_map; const uint16_t* left_map;  // dual only (m == nullptr: raw)
    uint32_t m_num_right;
};

namespace kern {

// ---- gen.hip: input contract, candidate generation, work lists
void validate_batch(uint32_t blocks, hipStream_t stream, const BatchArgs& a, uint64_t total_bytes);
void gen_candidates(uint32_t n, uint32_t lds_bytes, hipStream_t stream, const DevDict& D, const BatchArgs& a);
void build_lists(uint32_t blocks, hipStream_t stream, const BatchArgs& a, int only_list);
void gen_candidates_large(uint32_t workgroups, uint32_t waves, uint32_t lds_bytes, hipStream_t stream, const DevDict& D, const BatchArgs& a, uint32_t level);
void gen_set_max_lds(int bytes);  // hipFuncAttributeMaxDynamicSharedMemorySize of gen_candidates_large

// ---- lattice.hip: the sweep (one instance per {ignore_space, i32 matrix cells}) and the resident Worker kernel
void lattice_lds(uint32_t workgroups, uint32_t lds_bytes, hipStream_t stream, const DevDict& D, const BatchArgs& a, uint32_t tier, uint32_t persistent);
void lattice_set_max_lds(int bytes);
// the lean instance for whole sentences that arrive with the generator's pass records (built for 5 waves per SIMD); the common build only
bool lattice_has_lean();
void gen_sweep(uint32_t n, uint32_t lds_bytes, hipStream_t stream, const DevDict& D, const BatchArgs& a);  // generator + lean sweep in one wave (needs lattice_has_lean())
void lattice_lean(uint32_t workgroups, uint32_t lds_bytes, hipStream_t stream, const DevDict& D, const BatchArgs& a, uint32_t tier);
// the segment tier's instance without the C++ loop, the `exact` mode and connection-id counting (i16 cells, < 8000 characters, tier <= 64 KiB)
void lattice_slim(uint32_t workgroups, uint32_t lds_bytes, hipStream_t stream, const DevDict& D, const BatchArgs& a, uint32_t tier);
void tokenize_serve(uint32_t lds_bytes, hipStream_t stream, const DevDict& D, const BatchArgs& a, const uint8_t* h_text, uint32_t* ctl, uint32_t last_seq,
                    uint32_t idle_polls, uint32_t max_served);

// ---- fused.hip: the single-kernel fallback (global-memory lattice) and its LDS form (VBT_FUSED=1)
void fused_lds(uint32_t workgroups, uint32_t lds_bytes, hipStream_t stream, const DevDict& D, const BatchArgs& a, const uint32_t* in_list, const uint32_t* in_count,
               uint32_t* cursor, uint32_t* out_list, uint32_t* out_count);
void fused_global(uint32_t workgroups, hipStream_t stream, const DevDict& D, const BatchArgs& a, const uint32_t* in_list, const uint32_t* in_count, uint32_t* cursor);

// ---- nbest.hip: the K best paths per sentence (one wavefront per sentence, K sorted entries per node) and their pack pass
// nbest_lds: block b = sentence b, the arena in lds_bytes of LDS (0: everything is filed); out_list / out_count: what did not fit.
// nbest_slab: persistent waves over that list, arenas from a.scratch (bump pointer ctrl[kBump]).  nbest_pack: tile sums, their
// scan (nb.totals, path_off[n], tok_off[paths]) and the copy into sentence-major, rank-minor order.
void nbest_lds(uint32_t n, uint32_t lds_bytes, hipStream_t stream, const DevDict& D, const BatchArgs& a, const NBestArgs& nb, uint32_t* out_list, uint32_t* out_count);
void nbest_slab(uint32_t workgroups, hipStream_t stream, const DevDict& D, const BatchArgs& a, const NBestArgs& nb, const uint32_t* in_list, const uint32_t* in_count, uint32_t* cursor);
void nbest_pack(hipStream_t stream, const BatchArgs& a, const NBestArgs& nb);

// ---- marginal.hip: the posterior probability of every lattice node (forward-backward in float64, one wavefront per sentence)
// marginal_lds / marginal_slab: the tiers as nbest's; a sentence takes its range of m.stage with one atomic add and files itself in
// m.oflow_list when the range ends behind m.stage_cap (m.rerun: the second run of those, over that list with marginal_slab).
// marginal_pack: tile sums, their scan (m.totals, node_off[n]) and the copy into sentence order.
void marginal_lds(uint32_t n, uint32_t lds_bytes, hipStream_t stream, const DevDict& D, const BatchArgs& a, const MarginalArgs& m, uint32_t* out_list, uint32_t* out_count);
void marginal_slab(uint32_t workgroups, hipStream_t stream, const DevDict& D, const BatchArgs& a, const MarginalArgs& m, const uint32_t* in_list, const uint32_t* in_count, uint32_t* cursor);
void marginal_pack(hipStream_t stream, const BatchArgs& a, const MarginalArgs& m);

// ---- sample.hip: whole paths drawn from P(path) ~ exp(-cost / T) (the marginals' forward sweep, then backward sampling; one
// wavefront per sentence).  sample_lds / sample_slab: the tiers as marginal's; a sentence takes its range of p.stage with one
// atomic add.  sample_pack: tile sums, their scan (p.totals, path_off[n], tok_off[paths]) and the copy into sentence-major,
// sample-minor order.
void sample_lds(uint32_t n, uint32_t lds_bytes, hipStream_t stream, const DevDict& D, const BatchArgs& a, const SampleArgs& p, uint32_t* out_list, uint32_t* out_count);
void sample_slab(uint32_t workgroups, hipStream_t stream, const DevDict& D, const BatchArgs& a, const SampleArgs& p, const uint32_t* in_list, const uint32_t* in_count, uint32_t* cursor);
void sample_pack(hipStream_t stream, const BatchArgs& a, const SampleArgs& p);

// ---- pack.hip: token compaction, connector expansion
uint32_t pack_split();  // workgroups per packing tile
void tok_tile_scan(hipStream_t stream, const BatchArgs& a, uint32_t* tile_sums, uint32_t n_tiles);
void compact_tokens(hipStream_t stream, const BatchArgs& a, const uint32_t* tile_sums, uint32_t n_tiles, uint32_t scanned);
void compact_tokens_out(uint32_t workgroups, hipStream_t stream, const BatchArgs& a, const uint32_t* tile_sums, uint32_t n_tiles, vbt_token_rec* out_tokens,
                        uint32_t* out_off, uint32_t* out_cnt);
void expand_connector_i16(dim3 grid, const DevConnector& c, int16_t* out, uint32_t num_right, uint32_t num_left, uint32_t* range_flag);
void expand_connector_i32(dim3 grid, const DevConnector& c, int32_t* out, uint32_t num_right, uint32_t num_left, uint32_t* range_flag);
// dst[l][r] = src[inv_left[l]][inv_right[r]] (i16 cells, or i32 when `wide`): the matrix under a renumbering of the connection ids
void permute_matrix(hipStream_t stream, const void* src, void* dst, bool wide, const uint16_t* inv_left, const uint16_t* inv_right, uint32_t num_left, uint32_t num_right);

// ---- wakati.hip: the segmented text of a batch ("surface surface ...\n" per sentence, back to back) from the staging regions
// wakati_plan (line_len[n], bytes per tile) -> wakati_scan (tile_bytes[] -> exclusive prefix, line_off[n] = total; count_tokens: also
// ctrl[kTotal] from tile_sums[], for a batch whose records are not packed) -> wakati_render (line_off[0 .. n), the lines into out;
// a line that would end beyond out_cap sets kErrWakatiCap and is not written).  tile_bytes: n_tiles words, n_tiles = ceil(n / kScanTile).
uint32_t wakati_round();  // tokens per LDS round of wakati_render
void wakati_lines(hipStream_t stream, const BatchArgs& a, uint32_t n_tiles, uint32_t* line_len, uint64_t* tile_bytes, uint64_t* line_off, uint8_t* out,
                  uint64_t out_cap, bool count_tokens);
// wakati_scan alone: the prefix both text modes take over their tiles' bytes
void text_tile_scan(hipStream_t stream, const BatchArgs& a, uint64_t* tile_bytes, uint32_t n_tiles, uint64_t* line_off, bool count_tokens);

// ---- mecab.hip: the MeCab-format text of a batch ("surface \t feature \n" per token, "EOS\n" per sentence) from the staging regions
// and the feature table `f`.  mecab_plan (line_len[n] u64, bytes per tile) -> text_tile_scan -> mecab_render (line_off[0 .. n), the
// lines into out; a line that would end beyond out_cap, or of 4 GiB and more, sets kErrWakatiCap and is not written; line_off[n] is
// the exact total either way).  mecab_render_again: takes that flag back and renders once more, into another buffer or capacity;
// line_len / tile_bytes / the staging regions of the batch must be what mecab_lines left.
uint32_t mecab_round();  // tokens per LDS round of mecab_render
void mecab_lines(hipStream_t stream, const BatchArgs& a, const DevFeatures& f, uint32_t n_tiles, uint64_t* line_len, uint64_t* tile_bytes, uint64_t* line_off,
                 uint8_t* out, uint64_t out_cap, bool count_tokens);
void mecab_render_again(hipStream_t stream, const BatchArgs& a, const DevFeatures& f, uint32_t n_tiles, const uint64_t* line_len, const uint64_t* tile_bytes,
                        uint64_t* line_off, uint8_t* out, uint64_t out_cap);

// ---- detail.hip: the detail text of a batch (tokenize/src/main.rs:108-123: per token "surface \t feature \tlex_type=.. \tleft_id=..
// \tright_id=.. \tword_cost=.. \ttotal_cost=.. \n", "EOS\n" per sentence) from the staging regions, the feature table `f` and the
// word-parameter table `w`.  detail_plan -> text_tile_scan -> detail_render, with the buffers, the capacity rule and the flag of
// mecab_lines; detail_render_again as mecab_render_again.
uint32_t detail_round();  // tokens per LDS round of detail_render
void detail_lines(hipStream_t stream, const BatchArgs& a, const DevFeatures& f, const DevWordParams& w, uint32_t n_tiles, uint64_t* line_len, uint64_t* tile_bytes,
                  uint64_t* line_off, uint8_t* out, uint64_t out_cap, bool count_tokens);
void detail_render_again(hipStream_t stream, const BatchArgs& a, const DevFeatures& f, const DevWordParams& w, uint32_t n_tiles, const uint64_t* line_len,
                         const uint64_t* tile_bytes, uint64_t* line_off, uint8_t* out, uint64_t out_cap);

// ---- format.hip: the text of a batch in a compiled format (format.hpp) -- per sentence bos, the node / unk program per token, eos.
// format_index: the format's field index (index[rows][slots]) cut out of the feature blob `f`; exc[0] = rows on the exception list
// (the host parses them), exc[1 ..] those rows (rows + 1 words).  format_plan -> text_tile_scan -> format_render, with the buffers,
// the capacity rule and the flag of mecab_lines; format_render_again as mecab_render_again.  `w` is read only by a program with
// kFmtUsesParams.
void format_index(hipStream_t stream, const DevFeatures& f, uint32_t rows, const FmtProgram& prog, uint2* index, uint32_t* exc);
// index[exc[1 + i]][s] = patch[i][s] for the n_exc rows of the exception list: the entries the host made for them, in one launch
void format_patch(hipStream_t stream, uint2* index, const uint32_t* exc, const uint2* patch, uint32_t n_exc, uint32_t slots, uint32_t rows);
void format_lines(hipStream_t stream, const BatchArgs& a, const DevFeatures& f, const DevWordParams& w, const DevFormat& d, uint32_t n_tiles, uint64_t* line_len,
                  uint64_t* tile_bytes, uint64_t* line_off, uint8_t* out, uint64_t out_cap, bool count_tokens);
void format_render_again(hipStream_t stream, const BatchArgs& a, const DevFeatures& f, const DevWordParams& w, const DevFormat& d, uint32_t n_tiles,
                         const uint64_t* line_len, const uint64_t* tile_bytes, uint64_t* line_off, uint8_t* out, uint64_t out_cap);

// ---- split.hip: raw bytes cut into sentences (BufRead::lines(): '\n' and "\r\n" end a line) over tiles of VBT_SPLIT_TILE bytes.
// raw: 16-byte aligned, readable up to the next multiple of 16 behind len.  split_count (count pass + scan of the tiles): tiles[t]
// (one uint4 per tile of raw) = {'\n's, dropped bytes in front of tile t, ..}, info[0 .. 4) = {n, consumed, bytes of text, 1 when
// the last sentence is the unterminated tail of a `final` buffer}.  split_scatter, with those four values back from the host: the
// kept bytes of raw[0 .. consumed) into text (4-byte aligned), offsets[0 .. n] (consumed > 0: the caller launches nothing otherwise).
uint32_t split_tile();
void split_count(hipStream_t stream, const uint8_t* raw, uint32_t len, bool final, uint4* tiles, uint32_t* info);
void split_scatter(hipStream_t stream, const uint8_t* raw, uint32_t len, uint32_t consumed, const uint4* tiles, uint8_t* text, uint64_t* offsets, uint32_t n,
                   uint32_t text_bytes, bool tail);

// the calibration sample (Tokenizer::maybe_calibrate): up to `want` sentences spread evenly over the batch, copied into s_text / s_offs
// (s_offs[0 .. k], k = info[0] = the sentences whose text fits cap_bytes; s_src: want words of scratch), on `stream`
void sample_batch(hipStream_t stream, const uint8_t* text, const uint64_t* offsets, uint64_t n, uint64_t total_bytes, uint32_t want, uint64_t cap_bytes,
                  uint8_t* s_text, uint64_t* s_offs, uint32_t* s_src, uint32_t* info);

}  // namespace kern
}  // namespace vbt
