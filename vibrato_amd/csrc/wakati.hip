// Wakati output rendered on the device (tokenize/src/main.rs:96-103: the surfaces of a sentence joined by ' ', then '\n'): the
// text of the batch, tok_cnt[] and the {start_byte, end_byte} of the token records in the per-sentence staging regions are all
// on the device when the sweeps have joined, so the segmented text is written there -- bytes + tokens (+ one byte per empty
// sentence) instead of 24 bytes per token -- and the records need not be packed at all.  DESIGN.md section 3.9.
//
// wakati_plan (one workgroup per tile of kScanTile sentences): line_len[s] and the bytes of the tile.
// wakati_scan (one workgroup): exclusive prefix of the tiles' bytes, 64-bit (the output of a batch may exceed 4 GiB), the total.
// wakati_render (one workgroup per tile): line_off[], then the lines, output-stationary: a wave takes a round of up to
// kWakatiRound tokens of a sentence into an LDS table {output start, source start}, every lane owns one ALIGNED dword of the
// round's output span, finds the token of its first byte by binary search in the table and puts the dword together from the
// text and the separators -- full dwords leave as one aligned 32-bit store, the ragged head and tail of a span as byte stores.
#include "device_common.hpp"

namespace vbt {
namespace {

constexpr uint32_t kWakatiBlock = 1024, kWakatiWaves = kWakatiBlock / 64;  // 16 waves share a tile: 16 sentences in a row per wave
constexpr uint32_t kWakatiRound = VBT_WAKATI_ROUND;
static_assert(kScanTile <= kWakatiBlock && kScanTile % kWakatiWaves == 0, "a thread per sentence for the tile's scan");
static_assert(kWakatiRound % 64 == 0, "a round is loaded 64 tokens at a time");

// {start_byte, end_byte} of record k of the staging region that starts at `slot`: the third and fourth word of the 24-byte record
__device__ __forceinline__ uint2 load_span(const BatchArgs& A, size_t slot, uint32_t k) {
    return reinterpret_cast<const uint2*>(A.tok_stage)[3 * (slot + k) + 1];
}

// line_len[s] = bytes of the surfaces + one separator behind every token (' ', '\n' behind the last); "\n" for no tokens.
// (u32: a line is at most twice its sentence, and a workspace holds far less than 2 GiB of text -- ~400 bytes of device memory each)
__global__ void __launch_bounds__(kWakatiBlock) wakati_plan(BatchArgs A, uint32_t* __restrict__ line_len, uint64_t* __restrict__ tile_bytes) {
    __shared__ unsigned long long tile_total;
    if (A.ctrl[kError] & (uint32_t)kErrFatal) return;
    if (threadIdx.x == 0) tile_total = 0;
    __syncthreads();
    const uint32_t tile0 = blockIdx.x * kScanTile, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t o0 = A.offsets[0];
    unsigned long long mine = 0;
    for (uint32_t j = wave; j < kScanTile; j += kWakatiWaves) {
        const uint32_t s = tile0 + j;
        if (s >= A.n) break;
        const uint32_t nt = (uint32_t)__builtin_amdgcn_readfirstlane((int)A.tok_cnt[s]);
        const size_t slot = (size_t)(A.offsets[s] - o0) + (size_t)kSentenceSlack * s;
        uint32_t acc = 0;
        for (uint32_t k = lane; k < nt; k += 64) { const uint2 se = load_span(A, slot, k); acc += se.y - se.x; }
        const uint32_t len = wave_sum(acc) + (nt ? nt : 1u);
        if (lane == 0) line_len[s] = len;
        mine += len;
    }
    if (lane == 0 && mine) atomicAdd(&tile_total, mine);
    __syncthreads();
    if (threadIdx.x == 0) tile_bytes[blockIdx.x] = tile_total;
}

// tile_bytes[t] -> bytes of the tiles in front of tile t; line_off[n] = bytes of the whole output.  One workgroup: every thread
// adds up a run of tiles, the runs' prefix is taken out of LDS.  (One path for every batch size: a launch of its own costs the
// call ~3 us, adding the tiles up inside wakati_render would need this kernel anyway beyond a few thousand tiles.)
// count_tokens: the records are not packed for this batch, so the grand total of tile_sums[] is left in ctrl[kTotal] here.
// (Shared with the MeCab-format renderer, mecab.hip, through kern::text_tile_scan: the same prefix over its tiles' bytes.)
__global__ void __launch_bounds__(1024) wakati_scan(BatchArgs A, uint64_t* __restrict__ tile_bytes, uint32_t n_tiles, uint64_t* __restrict__ line_off,
                                                    uint32_t count_tokens) {
    __shared__ uint64_t part[1024];
    __shared__ uint32_t tokens;
    if (A.ctrl[kError] & (uint32_t)kErrFatal) return;
    if (threadIdx.x == 0) tokens = 0;
    const uint32_t per = (n_tiles + 1023u) / 1024u;
    const uint32_t t0 = min(threadIdx.x * per, n_tiles), t1 = min(t0 + per, n_tiles);
    uint64_t sum = 0;
    uint32_t ntok = 0;
    for (uint32_t t = t0; t < t1; ++t) { sum += tile_bytes[t]; if (count_tokens) ntok += A.tile_sums[t]; }
    part[threadIdx.x] = sum;
    __syncthreads();
    if (ntok) atomicAdd(&tokens, ntok);
    uint64_t base = 0, all = 0;
    for (uint32_t i = 0; i < 1024; ++i) { const uint64_t x = part[i]; base += i < threadIdx.x ? x : 0ull; all += x; }
    for (uint32_t t = t0; t < t1; ++t) { const uint64_t x = tile_bytes[t]; tile_bytes[t] = base; base += x; }
    __syncthreads();
    if (threadIdx.x == 0) {
        line_off[A.n] = all;
        if (count_tokens) A.ctrl[kTotal] = tokens;
    }
}

__global__ void __launch_bounds__(kWakatiBlock) wakati_render(BatchArgs A, const uint32_t* __restrict__ line_len, const uint64_t* __restrict__ tile_bytes,
                                                              uint64_t* __restrict__ line_off, uint8_t* __restrict__ out, uint64_t out_cap) {
    __shared__ uint32_t ws[kWakatiWaves];
    __shared__ uint32_t offs[kScanTile + 1];                  // exclusive line offsets of the tile's sentences, relative to the tile
    __shared__ uint32_t t_out[kWakatiWaves][kWakatiRound + 1];  // per wave: where each token of the round starts in the round's output (+ its end)
    __shared__ uint32_t t_src[kWakatiWaves][kWakatiRound];      // ... and where its surface starts in the sentence
    if (A.ctrl[kError] & (uint32_t)kErrFatal) return;
    const uint32_t tile0 = blockIdx.x * kScanTile, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t base = tile_bytes[blockIdx.x];
    {
        const uint32_t s = tile0 + threadIdx.x;
        const uint32_t len = threadIdx.x < kScanTile && s < A.n ? line_len[s] : 0u;
        uint32_t tot;
        const uint32_t ex = block_exscan(len, ws, tot);
        if (threadIdx.x < kScanTile) {
            offs[threadIdx.x] = ex;
            if (s < A.n) line_off[s] = base + ex;
        }
        if (threadIdx.x == 0) offs[kScanTile] = tot;
    }
    __syncthreads();
    const uint64_t o0 = A.offsets[0];
    uint32_t* const tab = t_out[wave];
    uint32_t* const src = t_src[wave];
    for (uint32_t j = wave; j < kScanTile; j += kWakatiWaves) {
        const uint32_t sn = tile0 + j;
        if (sn >= A.n) break;
        const uint32_t nt = (uint32_t)__builtin_amdgcn_readfirstlane((int)A.tok_cnt[sn]);
        const uint64_t line0 = base + offs[j], line1 = line0 + (offs[j + 1] - offs[j]);
        if (line1 > out_cap) {  // the line does not fit the output buffer: flagged, not written
            if (lane == 0) atomicOr(&A.ctrl[kError], (uint32_t)kErrWakatiCap);
            continue;
        }
        if (nt == 0) {
            if (lane == 0) out[line0] = (uint8_t)'\n';
            continue;
        }
        const uint64_t sb = A.offsets[sn];
        const uint8_t* __restrict__ txt = A.text + sb;
        const uint32_t last_byte = (uint32_t)(A.offsets[sn + 1] - sb) - 1u;  // (nt > 0: the sentence is not empty)
        const size_t slot = (size_t)(sb - o0) + (size_t)kSentenceSlack * sn;
        uint64_t at = line0;  // where the round's output starts
        for (uint32_t r0 = 0; r0 < nt; r0 += kWakatiRound) {
            const uint32_t m = min(kWakatiRound, nt - r0);
            uint32_t run = 0;  // bytes of the round's output: its surfaces + a separator behind each
            for (uint32_t c = 0; c < m; c += 64) {
                const uint32_t k = c + lane;
                const uint2 se = k < m ? load_span(A, slot, r0 + k) : make_uint2(0u, 0u);
                uint32_t chunk;
                const uint32_t ex = wave_exscan(k < m ? se.y - se.x + 1u : 0u, chunk);
                if (k < m) { tab[k] = run + ex; src[k] = se.x; }
                run += chunk;
            }
            if (lane == 0) tab[m] = run;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            run = (uint32_t)min((uint64_t)run, line1 - at);  // (never beyond the line the plan measured)
            const bool ends_line = r0 + m == nt;
            const uint64_t a0 = at & ~3ull;          // the aligned dword the span starts in
            const uint32_t head = (uint32_t)(at - a0);  // bytes of it in front of the span
            const uint32_t nd = (uint32_t)(((uint64_t)head + run + 3u) >> 2);
            for (uint32_t d = lane; d < nd; d += 64) {
                const int64_t rel0 = (int64_t)4 * d - head;  // byte 0 of this lane's dword, relative to the round's output
                const uint32_t first = rel0 < 0 ? 0u : (uint32_t)rel0;
                uint32_t lo = 0, hi = m;  // the token whose output holds byte `first`: the last one that starts at or before it
                while (lo + 1 < hi) { const uint32_t mid = (lo + hi) >> 1; if (tab[mid] <= first) lo = mid; else hi = mid; }
                uint32_t t = lo, word = 0, have = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int64_t rel = rel0 + b;
                    if (rel < 0 || rel >= (int64_t)run) continue;
                    while ((uint32_t)rel >= tab[t + 1]) ++t;  // (every token has at least its separator: at most three steps per dword)
                    const uint32_t in_tok = (uint32_t)rel - tab[t], surface = tab[t + 1] - tab[t] - 1u;
                    const uint32_t ch = in_tok < surface ? (uint32_t)txt[min(src[t] + in_tok, last_byte)] : (ends_line && t + 1 == m ? (uint32_t)'\n' : (uint32_t)' ');
                    word |= ch << (8 * b);
                    have |= 1u << b;
                }
                uint8_t* const to = out + a0 + (uint64_t)4 * d;
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

}  // namespace

namespace kern {

uint32_t wakati_round() { return kWakatiRound; }
void text_tile_scan(hipStream_t stream, const BatchArgs& a, uint64_t* tile_bytes, uint32_t n_tiles, uint64_t* line_off, bool count_tokens) {
    hipLaunchKernelGGL(vbt::wakati_scan, dim3(1), dim3(1024), 0, stream, a, tile_bytes, n_tiles, line_off, count_tokens ? 1u : 0u);
}
void wakati_lines(hipStream_t stream, const BatchArgs& a, uint32_t n_tiles, uint32_t* line_len, uint64_t* tile_bytes, uint64_t* line_off, uint8_t* out,
                  uint64_t out_cap, bool count_tokens) {
    if (n_tiles) hipLaunchKernelGGL(vbt::wakati_plan, dim3(n_tiles), dim3(kWakatiBlock), 0, stream, a, line_len, tile_bytes);
    text_tile_scan(stream, a, tile_bytes, n_tiles, line_off, count_tokens);
    if (n_tiles) hipLaunchKernelGGL(vbt::wakati_render, dim3(n_tiles), dim3(kWakatiBlock), 0, stream, a, line_len, tile_bytes, line_off, out, out_cap);
}

}  // namespace kern
}  // namespace vbt
