// Raw bytes cut into lines on the device, with the semantics of BufRead::lines() (tokenize/src/main.rs:78-80): a line ends at
// '\n', ONE '\r' directly in front of that '\n' goes with it, every other '\r' is text; what follows the last '\n' is the tail --
// the last sentence of a `final` buffer when it is not empty, left to the caller otherwise.  DESIGN.md section 3.4d.
//
// Two flags per byte: eol = (b == '\n'), drop = eol || (b == '\r' && next == '\n').  The kept bytes go to i - drops_before(i), and
// the '\n' at i ends sentence eols_before(i): offsets[eols_before(i) + 1] = i - drops_before(i).  Both prefixes are sums over the
// whole buffer, taken as reduce -> scan -> scatter over tiles of VBT_SPLIT_TILE bytes, so that no workgroup ever waits for another:
//   split_count_pass   (one workgroup per tile): {eols, drops, index behind the tile's last '\n'} of the tile.
//   split_scan_pass    (one workgroup): the tiles' exclusive prefixes in place, and {n, consumed, text bytes, tail} for the host, which
//                 needs n to pick a workspace and to size the grids of everything behind.
//   split_scatter_pass (one workgroup per tile): the flags once more, their prefix inside the tile, the kept bytes compacted in LDS at
//                 the alignment of their destination and stored as aligned dwords (bytes at the ragged head and tail), the offsets.
// A lane takes 16 bytes per load: the flags of a chunk are two 16-bit masks, from SWAR compares on its four dwords, counted with
// popcount; a workgroup of four waves loads its whole tile up front (four chunks per lane), scans the chunks' counts across the wave
// by DPP and across the tile through one LDS table.
#include "device_common.hpp"

namespace vbt {
namespace {

constexpr uint32_t kSplitTile = VBT_SPLIT_TILE, kSplitBlock = 256, kSplitWaves = kSplitBlock / 64;
constexpr uint32_t kSplitIters = kSplitTile / (16 * kSplitBlock);  // chunks per lane; chunk c = it * kSplitBlock + thread sits at byte 16 c of the tile
static_assert(kSplitIters * 16 * kSplitBlock == kSplitTile && kSplitTile < (1u << 16), "whole rounds of 16-byte chunks; a tile's counts fit 16 bits");

// bit k of the result = byte k of w equals the byte replicated in `pat` (exact: no borrow crosses a byte)
__device__ __forceinline__ uint32_t bytes_equal(uint32_t w, uint32_t pat) {
    const uint32_t x = w ^ pat;
    const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);  // 0x80 where the byte of x is zero
    return ((z >> 7) * 0x00204081u >> 21) & 0xFu;
}
__device__ __forceinline__ uint32_t chunk_equal(const uint4& v, uint32_t pat) {
    return bytes_equal(v.x, pat) | bytes_equal(v.y, pat) << 4 | bytes_equal(v.z, pat) << 8 | bytes_equal(v.w, pat) << 12;
}

// The chunks of this lane's tile and their flags.  Bytes at and beyond `len` read as 0 (the allocation is readable up to the next
// multiple of 16).  The byte behind a chunk is its right neighbour's first: bit 0 of that lane's eol mask, one DPP shift away; lane
// 63 has no neighbour in its wave -- the next wave, the next round or the next tile holds the byte -- and reads it from memory.
struct TileFlags { uint4 v[kSplitIters]; uint32_t eol[kSplitIters], drop[kSplitIters]; };
__device__ __forceinline__ void load_flags(const uint8_t* __restrict__ raw, uint32_t len, uint32_t tile0, TileFlags& f) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t behind[kSplitIters];
#pragma unroll
    for (uint32_t it = 0; it < kSplitIters; ++it) {
        const uint64_t pos = (uint64_t)tile0 + 16u * (it * kSplitBlock + threadIdx.x);
        f.v[it] = pos < len ? *reinterpret_cast<const uint4*>(raw + pos) : make_uint4(0u, 0u, 0u, 0u);
        behind[it] = lane == 63u && pos + 16u < len ? (uint32_t)raw[pos + 16u] : 0u;
    }
#pragma unroll
    for (uint32_t it = 0; it < kSplitIters; ++it) {
        const uint64_t pos = (uint64_t)tile0 + 16u * (it * kSplitBlock + threadIdx.x);
        if (pos < len && pos + 16u > len) {  // the buffer's last chunk: its bytes behind the end are not text
            const uint32_t have = len - (uint32_t)pos;
            uint32_t* w = &f.v[it].x;
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) w[k] = have >= 4 * k + 4 ? w[k] : have <= 4 * k ? 0u : w[k] & (0xFFFFFFFFu >> (8 * (4 * k + 4 - have)));
        }
        const uint32_t eol = chunk_equal(f.v[it], 0x0A0A0A0Au), cr = chunk_equal(f.v[it], 0x0D0D0D0Du);
        uint32_t next_eol = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)eol, 0x130, 0xF, 0xF, false) & 1u;  // wave_shl:1 -- lane i reads lane i + 1
        if (lane == 63u) next_eol = behind[it] == (uint32_t)'\n';
        f.eol[it] = eol;
        f.drop[it] = eol | (cr & (eol >> 1 | next_eol << 15));
    }
}

// Per tile, 16 bytes: .x '\n's, .y dropped bytes, .z index behind the tile's last '\n' (0: none); split_scan turns .x / .y into the
// counts of the tiles in front.
__global__ void __launch_bounds__(kSplitBlock) split_count_pass(const uint8_t* __restrict__ raw, uint32_t len, uint4* __restrict__ tiles) {
    __shared__ uint32_t sums[kSplitWaves], last[kSplitWaves];
    const uint32_t tile0 = blockIdx.x * kSplitTile, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    TileFlags f;
    load_flags(raw, len, tile0, f);
    uint32_t cnt = 0, behind_last = 0;
#pragma unroll
    for (uint32_t it = 0; it < kSplitIters; ++it) {
        cnt += (uint32_t)__popc(f.eol[it]) | (uint32_t)__popc(f.drop[it]) << 16;
        if (f.eol[it]) behind_last = tile0 + 16u * (it * kSplitBlock + threadIdx.x) + (32u - (uint32_t)__clz((int)f.eol[it]));  // (chunks in ascending order)
    }
    cnt = wave_sum(cnt);
    behind_last = wave_umax(behind_last);
    if (lane == 0) { sums[wave] = cnt; last[wave] = behind_last; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0, l = 0;
        for (uint32_t w = 0; w < kSplitWaves; ++w) { c += sums[w]; l = max(l, last[w]); }
        tiles[blockIdx.x] = make_uint4(c & 0xFFFFu, c >> 16, l, 0u);
    }
}

// info[0 .. 4) = {n, consumed, bytes of the sentences' text, 1 when the last sentence is an unterminated tail}
__global__ void __launch_bounds__(1024) split_scan_pass(uint4* __restrict__ tiles, uint32_t n_tiles, uint32_t len, uint32_t final, uint32_t* __restrict__ info) {
    __shared__ uint32_t ws[16], behind_last;
    if (threadIdx.x == 0) behind_last = 0;
    const uint32_t per = (n_tiles + 1023u) / 1024u;
    const uint32_t t0 = min(threadIdx.x * per, n_tiles), t1 = min(t0 + per, n_tiles);
    uint32_t eols = 0, drops = 0, l = 0;
    for (uint32_t t = t0; t < t1; ++t) { const uint4 c = tiles[t]; eols += c.x; drops += c.y; l = max(l, c.z); }
    uint32_t all_eols, all_drops;
    uint32_t e = block_exscan(eols, ws, all_eols);  // (its first barrier is behind the store of behind_last)
    uint32_t d = block_exscan(drops, ws, all_drops);
    if (l) atomicMax(&behind_last, l);
    for (uint32_t t = t0; t < t1; ++t) { const uint4 c = tiles[t]; tiles[t] = make_uint4(e, d, c.z, 0u); e += c.x; d += c.y; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t tail = final && behind_last < len ? 1u : 0u;
        const uint32_t consumed = final ? len : behind_last;
        info[0] = all_eols + tail; info[1] = consumed; info[2] = consumed - all_drops; info[3] = tail;  // (every dropped byte lies in front of the last '\n')
    }
}

// limit: the bytes behind it are no sentence's text (== consumed).  text / offsets: 4- and 8-byte aligned; offsets[0 .. n].
__global__ void __launch_bounds__(kSplitBlock) split_scatter_pass(const uint8_t* __restrict__ raw, uint32_t len, uint32_t limit, const uint4* __restrict__ tiles,
                                                             uint8_t* __restrict__ text, uint64_t* __restrict__ offsets, uint32_t n, uint32_t text_bytes, uint32_t tail) {
    __shared__ uint32_t sums[kSplitIters * kSplitWaves];
    __shared__ __attribute__((aligned(4))) uint8_t kept[kSplitTile + 4];  // kept[k] goes to text[(first & ~3) + k], first = the tile's first destination
    const uint32_t tile0 = blockIdx.x * kSplitTile, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint4 before = tiles[blockIdx.x];
    TileFlags f;
    load_flags(raw, len, tile0, f);
    uint32_t ex[kSplitIters];
#pragma unroll
    for (uint32_t it = 0; it < kSplitIters; ++it) {
        uint32_t tot;
        ex[it] = wave_exscan((uint32_t)__popc(f.eol[it]) | (uint32_t)__popc(f.drop[it]) << 16, tot);
        if (lane == 0) sums[it * kSplitWaves + wave] = tot;
    }
    __syncthreads();
    const uint32_t first = tile0 - before.y, head = first & 3u;
    uint32_t run = 0;  // counts of the rounds in front of this lane's next chunk
#pragma unroll
    for (uint32_t it = 0; it < kSplitIters; ++it) {
        uint32_t base = run;
#pragma unroll
        for (uint32_t w = 0; w < kSplitWaves; ++w) { const uint32_t s = sums[it * kSplitWaves + w]; base += w < wave ? s : 0u; run += s; }
        base += ex[it];
        const uint32_t off = 16u * (it * kSplitBlock + threadIdx.x), pos = tile0 + off;  // (pos may wrap behind a buffer of nearly 4 GiB: such a chunk has no flags and no bytes)
        const uint32_t have = (uint64_t)tile0 + off < limit ? min(16u, limit - pos) : 0u;
        const uint32_t keep = ((1u << have) - 1u) & ~f.drop[it];
        uint32_t at = head + off - (base >> 16);
        const uint32_t* w = &f.v[it].x;
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k)
            if (keep >> k & 1u) kept[at++] = (uint8_t)(w[k >> 2] >> (8 * (k & 3u)));
        uint32_t e = before.x + (base & 0xFFFFu) + 1u;
        for (uint32_t m = f.eol[it]; m; m &= m - 1u) {
            const uint32_t k = (uint32_t)__ffs((int)m) - 1u;
            offsets[e++] = (uint64_t)(pos + k - before.y - (base >> 16) - (uint32_t)__popc(f.drop[it] & ((1u << k) - 1u)));
        }
    }
    __syncthreads();
    const uint32_t span = head + min(kSplitTile, limit - tile0) - (run >> 16);  // the tile's bytes in front of the limit without the dropped ones (all in front of it)
    uint8_t* const to = text + (first - head);
    for (uint32_t q = threadIdx.x; 4u * q < span; q += kSplitBlock) {
        const uint32_t lo = 4u * q;
        if (lo >= head && lo + 4u <= span) *reinterpret_cast<uint32_t*>(to + lo) = *reinterpret_cast<const uint32_t*>(kept + lo);
        else {
#pragma unroll
            for (uint32_t b = 0; b < 4; ++b)
                if (lo + b >= head && lo + b < span) to[lo + b] = kept[lo + b];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        offsets[0] = 0;
        if (tail) offsets[n] = text_bytes;
    }
}

}  // namespace

namespace kern {

uint32_t split_tile() { return kSplitTile; }
void split_count(hipStream_t stream, const uint8_t* raw, uint32_t len, bool final, uint4* tiles, uint32_t* info) {
    const uint32_t n_tiles = (uint32_t)(((uint64_t)len + kSplitTile - 1) / kSplitTile);
    hipLaunchKernelGGL(vbt::split_count_pass, dim3(n_tiles), dim3(kSplitBlock), 0, stream, raw, len, tiles);
    hipLaunchKernelGGL(vbt::split_scan_pass, dim3(1), dim3(1024), 0, stream, tiles, n_tiles, len, final ? 1u : 0u, info);
}
void split_scatter(hipStream_t stream, const uint8_t* raw, uint32_t len, uint32_t limit, const uint4* tiles, uint8_t* text, uint64_t* offsets, uint32_t n,
                   uint32_t text_bytes, bool tail) {
    const uint32_t n_tiles = (uint32_t)(((uint64_t)limit + kSplitTile - 1) / kSplitTile);
    hipLaunchKernelGGL(vbt::split_scatter_pass, dim3(n_tiles), dim3(kSplitBlock), 0, stream, raw, len, limit, tiles, text, offsets, n, text_bytes, tail ? 1u : 0u);
}

}  // namespace kern
}  // namespace vbt
