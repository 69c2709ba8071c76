// reply_common.h -- what the two reply kernels share: k_reply
// (reply_kernels.hip, fws_gpu_reply_messages_multi) and k_reply_strict
// (reply_strict_kernels.hip, fws_gpu_reply_messages_strict). The compacted
// frame table of one read in LDS, the search that finds a region offset's
// frame in it, and the seam-chunk builder over it (tx_multi_common.h holds the
// byte builders themselves).
#pragma once

#include "fws_device.h"
#include "tx_multi_common.h"

namespace fwsk {

constexpr uint32_t kRpItems = FWS_MSG_MULTI_MAX_FRAMES + 2u;   // the entries (a lead's and one per header), the open part
constexpr uint32_t kRpNone = 0xFFFFFFFFu;

// the frame table (compacted: frame j of the region)
struct RpTable {
    uint64_t src[kRpItems];        // address of the payload's first byte
    uint32_t off[kRpItems];        // the header's offset in the region
    uint32_t len[kRpItems];        // payload bytes
    uint32_t bh[kRpItems];         // b0 | header bytes << 8
};

__device__ __forceinline__ TmFrame rp_frame(const RpTable &t, uint32_t j) {
    TmFrame f;
    f.O = t.off[j];
    f.plen = t.len[j];
    f.hlen = t.bh[j] >> 8;
    f.b0 = t.bh[j] & 0xFFu;
    f.P = f.O + f.hlen;
    f.E = f.P + f.plen;
    f.soff = 0u;
    f.key = 0u;
    return f;
}

// the frame holding region offset a (< total): the last one whose offset is <= a
__device__ __forceinline__ uint32_t rp_frame_of(const RpTable &t, uint32_t nf, uint32_t a) {
    uint32_t lo = 0u, hi = nf - 1u;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1u) >> 1);
        if (t.off[mid] <= a) lo = mid; else hi = mid - 1u;
    }
    return lo;
}

// tm_seam_chunk over the table: every frame from j on that meets [a, a + 16)
// gives its header bytes and its payload bytes; bytes at or past the total stay
// zero. A source block that holds no byte of the frame's payload is replaced by
// one that does (its bytes are never selected), so every load is in bounds.
__device__ u32x4 rp_seam_chunk(const RpTable &t, uint32_t nf, uint32_t a, uint32_t j) {
    u32x4 x{0u, 0u, 0u, 0u};
    for (; j < nf; ++j) {
        const TmFrame f = rp_frame(t, j);
        if (f.O >= a + 16u) break;
        const uint32_t ho = tm_rel(f.O, a), hp = tm_rel(f.P, a), he = tm_rel(f.E, a);
        if (hp > ho) {                                 // -16 < a - O < 16: the header is 10 bytes at most
            const int off = (int)a - (int)f.O;
            if (off > -16 && off < 16) x = x | tm_and_sel(tm_bytes_at(tm_hdr_vec(f, false), off), ho, hp);
        }
        if (he > hp) {
            const uintptr_t s0 = (uintptr_t)t.src[j], s1 = s0 + f.plen;
            const uintptr_t sa = s0 + (uintptr_t)a - (uintptr_t)f.P;
            const uintptr_t safe = s0 & ~uintptr_t(15);
            uintptr_t b0 = sa & ~uintptr_t(15), b1 = b0 + 16u;
            if (b0 + 16u <= s0 || b0 >= s1) b0 = safe;
            if (b1 + 16u <= s0 || b1 >= s1) b1 = safe;
            const u32x4 w = tm_shr_bytes(gload16<false>(b0), gload16<false>(b1), (uint32_t)(sa & 15u));
            x = x | tm_and_sel(w, hp, he);
        }
    }
    return x;
}

}  // namespace fwsk
