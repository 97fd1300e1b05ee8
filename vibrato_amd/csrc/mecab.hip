// MeCab-format output rendered on the device (tokenize/src/main.rs:83-95: "surface \t feature \n" per token, then "EOS\n"; "EOS\n"
// alone for a sentence without tokens).  Everything the host formatter reads is on the device when the sweeps have joined: the text,
// tok_cnt[], {start_byte, end_byte, word_idx} of the staged records, and the feature strings as one static blob of the dictionary
// (DevFeatures, uploaded when a workspace first asks for this mode).  DESIGN.md section 3.4b.
//
// Unlike a wakati line, a MeCab line interleaves TWO sources -- sentence bytes and feature bytes, 40-150 of the latter per token --
// and its length is not bounded by its sentence, so every size here is 64-bit until it is known to fit, and the caller names the
// capacity of the output buffer.
//
// mecab_plan (one workgroup per tile of kScanTile sentences): line_len[s] (u64) and the bytes of the tile.
// text_tile_scan (wakati.hip, shared): exclusive prefix of the tiles' bytes, line_off[n] = the exact total, whatever the capacity.
// mecab_render (one workgroup per tile): line_off[], then the lines, output-stationary: a wave takes a round of up to kMecabRound
// tokens into an LDS piece table {output start, surface start, surface length, feature offset in the blob}; every lane owns one
// ALIGNED dword of the round's output span and finds the token of its first byte by binary search in the output starts.  A dword
// that lies inside one feature string -- the common case -- is fetched with two aligned dword loads of the blob and a byte-align;
// everything else (surfaces, '\t', '\n', token borders, "EOS\n", the ragged ends of the span) is put together byte by byte.  Full
// dwords leave as one aligned 32-bit store, only the ragged first and last dword of a span as byte stores.  Nothing is sized by the
// longest sentence or feature: more tokens than a round loop over rounds, more dwords than 64 loop over the lanes.
// (detail.hip is this scheme with a longer piece table: the decimal fields of a detail line are further pieces of a token's span.)
#include "text_pieces.hpp"  // Piece, load_piece, wave_sum64: shared with detail.hip

namespace vbt {
namespace {

constexpr uint32_t kMecabBlock = 1024, kMecabWaves = kMecabBlock / 64;  // 16 waves share a tile: 16 sentences in a row per wave
constexpr uint32_t kMecabRound = VBT_MECAB_ROUND;
static_assert(kScanTile <= kMecabBlock && kScanTile % kMecabWaves == 0 && kScanTile % 64 == 0, "a thread per sentence for the tile's scan");
static_assert(kMecabRound % 64 == 0, "a round is loaded 64 tokens at a time");
static_assert(kMecabWaves * (4 * kMecabRound + 1) * 4 + (kScanTile + 1 + kScanTile / 64) * 8 <= 65536, "the piece tables and the tile's offsets within 64 KiB of LDS");

// line_len[s] = per token its surface + '\t' + its feature + '\n', then "EOS\n"
__global__ void __launch_bounds__(kMecabBlock) mecab_plan(BatchArgs A, DevFeatures F, uint64_t* __restrict__ line_len, uint64_t* __restrict__ tile_bytes) {
    __shared__ unsigned long long tile_total;
    if (A.ctrl[kError] & (uint32_t)kErrFatal) return;
    if (threadIdx.x == 0) tile_total = 0;
    __syncthreads();
    const uint32_t tile0 = blockIdx.x * kScanTile, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t o0 = A.offsets[0];
    unsigned long long mine = 0;
    for (uint32_t j = wave; j < kScanTile; j += kMecabWaves) {
        const uint32_t s = tile0 + j;
        if (s >= A.n) break;
        const uint32_t nt = (uint32_t)__builtin_amdgcn_readfirstlane((int)A.tok_cnt[s]);
        const size_t slot = (size_t)(A.offsets[s] - o0) + (size_t)kSentenceSlack * s;
        uint64_t acc = 0;
        for (uint32_t k = lane; k < nt; k += 64) {
            const Piece p = load_piece(A, F, slot, k);
            acc += (uint64_t)(p.end - p.start) + p.feat_len + 2u;
        }
        const uint64_t len = wave_sum64(acc) + 4u;
        if (lane == 0) line_len[s] = len;
        mine += len;
    }
    if (lane == 0 && mine) atomicAdd(&tile_total, mine);
    __syncthreads();
    if (threadIdx.x == 0) tile_bytes[blockIdx.x] = tile_total;
}

__global__ void __launch_bounds__(kMecabBlock) mecab_render(BatchArgs A, DevFeatures F, const uint64_t* __restrict__ line_len, const uint64_t* __restrict__ tile_bytes,
                                                            uint64_t* __restrict__ line_off, uint8_t* __restrict__ out, uint64_t out_cap) {
    __shared__ uint64_t wsum[kScanTile / 64];
    __shared__ uint64_t offs[kScanTile + 1];                     // exclusive line offsets of the tile's sentences, relative to the tile
    __shared__ uint32_t t_out[kMecabWaves][kMecabRound + 1];     // per wave, per token of the round: where its output starts in the round's span (+ the end)
    __shared__ uint32_t t_src[kMecabWaves][kMecabRound];         // where its surface starts in the sentence
    __shared__ uint32_t t_len[kMecabWaves][kMecabRound];         // bytes of its surface
    __shared__ uint32_t t_feat[kMecabWaves][kMecabRound];        // where its feature starts in the blob
    if (A.ctrl[kError] & (uint32_t)kErrFatal) return;
    const uint32_t tile0 = blockIdx.x * kScanTile, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t base = tile_bytes[blockIdx.x];
    {   // 64-bit exclusive prefix of the tile's line lengths: the first kScanTile threads, a sentence each
        const uint32_t s = tile0 + threadIdx.x;
        const bool in_tile = threadIdx.x < kScanTile;
        const uint64_t len = in_tile && s < A.n ? line_len[s] : 0ull;
        uint64_t inc = len;
        if (in_tile) {  // (whole waves: kScanTile is a multiple of 64)
            for (uint32_t o = 1; o < 64; o <<= 1) { const uint64_t u = __shfl_up(inc, o); if (lane >= o) inc += u; }
            if (lane == 63) wsum[wave] = inc;
        }
        __syncthreads();
        if (in_tile) {
            uint64_t front = 0;
            for (uint32_t i = 0; i < wave; ++i) front += wsum[i];
            offs[threadIdx.x] = front + inc - len;
            if (s < A.n) line_off[s] = base + front + inc - len;
            if (threadIdx.x == kScanTile - 1) offs[kScanTile] = front + inc;
        }
    }
    __syncthreads();
    const uint64_t o0 = A.offsets[0];
    const uint32_t* __restrict__ blob32 = reinterpret_cast<const uint32_t*>(F.blob);
    uint32_t* const tab = t_out[wave];
    uint32_t* const src = t_src[wave];
    uint32_t* const slen = t_len[wave];
    uint32_t* const feat = t_feat[wave];
    for (uint32_t j = wave; j < kScanTile; j += kMecabWaves) {
        const uint32_t sn = tile0 + j;
        if (sn >= A.n) break;
        const uint32_t nt = (uint32_t)__builtin_amdgcn_readfirstlane((int)A.tok_cnt[sn]);
        const uint64_t line0 = base + offs[j], len = offs[j + 1] - offs[j], line1 = line0 + len;
        if (len >= (1ull << 32) || line1 > out_cap) {  // the line does not fit the output buffer (or 32-bit sizes): flagged, not written
            if (lane == 0) atomicOr(&A.ctrl[kError], (uint32_t)kErrWakatiCap);
            continue;
        }
        const uint64_t sb = A.offsets[sn];
        const uint8_t* __restrict__ txt = A.text + sb;
        const uint32_t nb = (uint32_t)(A.offsets[sn + 1] - sb);
        const uint32_t last_byte = nb ? nb - 1u : 0u;  // (only read when a token has a surface: the sentence is not empty then)
        const size_t slot = (size_t)(sb - o0) + (size_t)kSentenceSlack * sn;
        uint64_t at = line0;  // where the round's output starts
        // (a sentence without tokens: one round without pieces, its span the four bytes of "EOS\n")
        for (uint32_t r0 = 0; r0 < nt || r0 == 0; r0 += kMecabRound) {
            const uint32_t m = min(kMecabRound, nt - r0);
            uint32_t run = 0;  // bytes of the round's pieces
            for (uint32_t c = 0; c < m; c += 64) {
                const uint32_t k = c + lane;
                Piece p{0u, 0u, 0u, 0u};
                if (k < m) p = load_piece(A, F, slot, r0 + k);
                uint32_t chunk;
                const uint32_t ex = wave_exscan(k < m ? p.end - p.start + p.feat_len + 2u : 0u, chunk);
                if (k < m) { tab[k] = run + ex; src[k] = p.start; slen[k] = p.end - p.start; feat[k] = p.feat; }
                run += chunk;
            }
            if (lane == 0) tab[m] = run;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const uint32_t pieces = run;                 // "EOS\n" sits behind the pieces of the line's last round
            const bool ends_line = r0 + m == nt;
            if (ends_line) run += 4u;
            run = (uint32_t)min((uint64_t)run, line1 - at);  // (never beyond the line the plan measured)
            const uint64_t a0 = at & ~3ull;              // the aligned dword the span starts in
            const uint32_t head = (uint32_t)(at - a0);   // bytes of it in front of the span
            const uint32_t nd = (uint32_t)(((uint64_t)head + run + 3u) >> 2);
            for (uint32_t d = lane; d < nd; d += 64) {
                const int64_t rel0 = (int64_t)4 * d - head;  // byte 0 of this lane's dword, relative to the round's output
                const uint32_t first = rel0 < 0 ? 0u : (uint32_t)rel0;
                uint32_t lo = 0, hi = m;  // the token whose output holds byte `first`: the last one that starts at or before it
                while (lo + 1 < hi) { const uint32_t mid = (lo + hi) >> 1; if (tab[mid] <= first) lo = mid; else hi = mid; }
                uint32_t t = lo, word = 0, have = 0;
                uint8_t* const to = out + a0 + (uint64_t)4 * d;
                if (m && rel0 >= 0 && (uint64_t)rel0 + 4u <= run) {
                    // all four bytes inside the feature of token t?  feature bytes are [tab[t] + surface + 1, tab[t + 1] - 1)
                    const uint32_t f_begin = tab[t] + slen[t] + 1u, f_end = tab[t + 1] - 1u;
                    if (first >= f_begin && first + 4u <= f_end) {
                        const uint32_t addr = feat[t] + (first - f_begin);  // absolute in the blob, + 3 inside this feature
                        const uint32_t w0 = blob32[addr >> 2], w1 = blob32[(addr >> 2) + 1];  // (w1: at most the blob's zero slack)
                        *reinterpret_cast<uint32_t*>(to) = __builtin_amdgcn_alignbyte(w1, w0, addr & 3u);
                        continue;
                    }
                }
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int64_t rel = rel0 + b;
                    if (rel < 0 || rel >= (int64_t)run) continue;
                    const uint32_t r = (uint32_t)rel;
                    uint32_t ch;
                    if (r >= pieces) ch = (0x0A534F45u >> (8u * ((r - pieces) & 3u))) & 0xFFu;  // "EOS\n"
                    else {
                        while (r >= tab[t + 1]) ++t;  // (every token has at least its '\t' and '\n': at most two steps per dword)
                        const uint32_t in_tok = r - tab[t], sl = slen[t];
                        if (in_tok < sl) ch = (uint32_t)txt[min(src[t] + in_tok, last_byte)];
                        else if (in_tok == sl) ch = (uint32_t)'\t';
                        else if (r + 1u == tab[t + 1]) ch = (uint32_t)'\n';
                        else ch = (uint32_t)F.blob[feat[t] + (in_tok - sl - 1u)];
                    }
                    word |= ch << (8 * b);
                    have |= 1u << b;
                }
                if (have == 0xFu) *reinterpret_cast<uint32_t*>(to) = word;
                else {
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (have >> b & 1u) to[b] = (uint8_t)(word >> (8 * b));
                }
            }
            at += run;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the table is rewritten by the next round)
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// Workspace::render_text_again: the capacity flag of the run is taken back before the lines are rendered into a larger buffer
__global__ void mecab_clear_cap_flag(uint32_t* ctrl) { atomicAnd(&ctrl[kError], ~(uint32_t)kErrWakatiCap); }

}  // namespace

namespace kern {

uint32_t mecab_round() { return kMecabRound; }
void mecab_lines(hipStream_t stream, const BatchArgs& a, const DevFeatures& f, uint32_t n_tiles, uint64_t* line_len, uint64_t* tile_bytes, uint64_t* line_off,
                 uint8_t* out, uint64_t out_cap, bool count_tokens) {
    if (n_tiles) hipLaunchKernelGGL(vbt::mecab_plan, dim3(n_tiles), dim3(kMecabBlock), 0, stream, a, f, line_len, tile_bytes);
    text_tile_scan(stream, a, tile_bytes, n_tiles, line_off, count_tokens);
    if (n_tiles) hipLaunchKernelGGL(vbt::mecab_render, dim3(n_tiles), dim3(kMecabBlock), 0, stream, a, f, line_len, tile_bytes, line_off, out, out_cap);
}
void mecab_render_again(hipStream_t stream, const BatchArgs& a, const DevFeatures& f, uint32_t n_tiles, const uint64_t* line_len, const uint64_t* tile_bytes,
                        uint64_t* line_off, uint8_t* out, uint64_t out_cap) {
    hipLaunchKernelGGL(vbt::mecab_clear_cap_flag, dim3(1), dim3(1), 0, stream, a.ctrl);
    if (n_tiles) hipLaunchKernelGGL(vbt::mecab_render, dim3(n_tiles), dim3(kMecabBlock), 0, stream, a, f, line_len, tile_bytes, line_off, out, out_cap);
}

}  // namespace kern
}  // namespace vbt
