// tx_multi_common.h -- the byte builders shared by the kernels that write
// frames back to back into a region in 16-B chunks: k_tx_multi
// (tx_multi_kernels.hip, regular frames found by a division) and k_reply
// (reply_kernels.hip, irregular frames found by a search). A chunk inside one
// payload is two aligned source loads shifted by the source misalignment; a
// chunk that meets a header or the region's end (a seam) ORs, for every frame
// that meets it, the header from registers and the source window, each selected
// on its byte range.
#pragma once

#include "fws_device.h"

namespace fwsk {

constexpr uint32_t kTmU = 4;                 // chunks per thread per round (8 loads in flight)

struct TmFrame {
    uint32_t O, P, E;      // header, payload and end offsets in the region
    uint32_t plen, hlen, soff, key, b0;
};

__device__ __forceinline__ uint32_t tm_hdr_len(uint32_t p, bool masked) {   // w_socket.h:49-65
    return 2u + (masked ? 4u : 0u) + (p < 126u ? 0u : (p <= 65535u ? 2u : 8u));
}

// 16 bytes starting sh (0..15) bytes into the 32-byte window v0:v1 (tx_kernels.hip)
__device__ __forceinline__ u32x4 tm_shr_bytes(const u32x4 &v0, const u32x4 &v1, uint32_t sh) {
    const bool s8 = (sh & 8u) != 0, s4 = (sh & 4u) != 0;
    const uint32_t a0 = s8 ? v0.z : v0.x, a1 = s8 ? v0.w : v0.y, a2 = s8 ? v1.x : v0.z;
    const uint32_t a3 = s8 ? v1.y : v0.w, a4 = s8 ? v1.z : v1.x;
    const uint32_t c0 = s4 ? a1 : a0, c1 = s4 ? a2 : a1, c2 = s4 ? a3 : a2, c3 = s4 ? a4 : a3;
    const uint32_t c4 = s4 ? (s8 ? v1.w : v1.y) : a4;
    const uint32_t b = sh & 3u;
    return u32x4{__builtin_amdgcn_alignbyte(c1, c0, b), __builtin_amdgcn_alignbyte(c2, c1, b),
                 __builtin_amdgcn_alignbyte(c3, c2, b), __builtin_amdgcn_alignbyte(c4, c3, b)};
}

// 16 bytes of v as seen from byte offset off (-16 < off < 16): byte i of the
// result is v's byte i + off, zero outside v.
__device__ __forceinline__ u32x4 tm_bytes_at(const u32x4 &v, int off) {
    const u32x4 z{0u, 0u, 0u, 0u};
    return off >= 0 ? tm_shr_bytes(v, z, (uint32_t)off) : tm_shr_bytes(z, v, (uint32_t)(16 + off));
}

// The frame header as 16 bytes (<= 14 used, rest zero), little-endian dwords:
// b0, b1, the big-endian 16 / 64-bit length, then the key bytes (masked frames).
__device__ __forceinline__ u32x4 tm_hdr_vec(const TmFrame &f, bool masked) {
    const uint32_t m = masked ? 0x80u : 0u, k = f.key, L = f.plen;
    if (L < 126u) return u32x4{f.b0 | ((m | L) << 8) | ((k & 0xFFFFu) << 16), k >> 16, 0u, 0u};
    if (L <= 65535u)
        return u32x4{f.b0 | ((m | 126u) << 8) | (((L >> 8) & 0xFFu) << 16) | ((L & 0xFFu) << 24), k, 0u, 0u};
    const uint32_t lo = __builtin_bswap32(L);          // bytes 2..9 = L big endian, its high dword zero
    return u32x4{f.b0 | ((m | 127u) << 8), lo << 16, (lo >> 16) | ((k & 0xFFFFu) << 16), k >> 16};
}

// x clipped to [a, a + 16), as an offset from a
__device__ __forceinline__ uint32_t tm_rel(uint32_t x, uint32_t a) {
    return x <= a ? 0u : (x >= a + 16u ? 16u : x - a);
}

// Byte-select mask of the chunk's bytes [lo, hi) (offsets 0..16) for dword i
__device__ __forceinline__ uint32_t tm_sel(uint32_t lo, uint32_t hi, uint32_t i) {
    const uint32_t o = 4u * i;
    if (hi <= o || lo >= o + 4u) return 0u;
    const uint32_t s = lo > o ? lo - o : 0u, e = hi < o + 4u ? o + 4u - hi : 0u;
    return (0xFFFFFFFFu << (8u * s)) & (0xFFFFFFFFu >> (8u * e));
}

__device__ __forceinline__ u32x4 tm_and_sel(const u32x4 &v, uint32_t lo, uint32_t hi) {
    return u32x4{v.x & tm_sel(lo, hi, 0), v.y & tm_sel(lo, hi, 1), v.z & tm_sel(lo, hi, 2), v.w & tm_sel(lo, hi, 3)};
}

// region bytes [a, min(a + 16, total)) of x
__device__ __forceinline__ void tm_store_chunk(uint8_t *__restrict__ R, uint32_t a, uint32_t total, const u32x4 &x) {
    if (a + 16u <= total) {
        gstore16<true>((uintptr_t)(R + a), x);
        return;
    }
    const uint32_t nb = total - a;
    const uint32_t xw[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (uint32_t i = 0; i < 16u; ++i)                 // (static indices: no scratch)
        if (i < nb) gput(R + a + i, (uint8_t)(xw[i >> 2] >> (8u * (i & 3u))));
}

}  // namespace fwsk
