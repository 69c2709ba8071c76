// reply_common.h -- what the two reply kernels share: k_reply
// (reply_kernels.hip, fws_gpu_reply_messages_multi) and k_reply_strict
// (reply_strict_kernels.hip, fws_gpu_reply_messages_strict). The result
// writer, the workgroup scan that gives each frame its index and offset, the
// compacted frame table of one read in LDS, the search that finds a region
// offset's frame in it, the seam-chunk builder over it (tx_multi_common.h holds
// the byte builders themselves), the byte phase and the frame records. The
// classification of the items and the table fill stay with each kernel.
//
// kMasked: the client form (fws_gpu_reply_messages_*_client). Every frame has
// the MASK bit and a key, FWS_TX_FRAG_KEY(key0, j) for frame j of the region
// (key0: the read's word of dev_keys), so the key is a function of the frame
// index the table search already gives and the table holds none. The payload
// is XORed from phase 0: a 4-aligned dword at region offset av of a frame whose
// payload starts at P takes the key rotated to (av - P) & 3. With kMasked false
// key0 is unused and the code is what it was.
#pragma once

#include "fws_device.h"
#include "tx_multi_common.h"

namespace fwsk {

constexpr uint32_t kRpItems = FWS_MSG_MULTI_MAX_FRAMES + 2u;   // the entries (a lead's and one per header), the open part
constexpr uint32_t kRpNone = 0xFFFFFFFFu;

__device__ __forceinline__ void rp_result(fws_tx_result *res, uint32_t r, int32_t status, uint32_t n_frames,
                                          uint64_t out_len, uint32_t lmnf) {
    fws_tx_result x{};
    x.status = status;
    x.n_frames = n_frames;
    x.out_len = out_len;
    x.last_msg_not_fin = lmnf;
    gput(res + r, x);
}

// Frame index and offset: the workgroup scan of a thread's (frames, bytes) over
// its consecutive items. pc / pb: frames / bytes before the thread's first item;
// nf / total: the read's (a frame is at most 128 KiB + 14 and there are fewer
// than 260: under 2^26, no overflow). s_wc / s_wb: kWaves words each; passes one
// barrier.
struct RpScan {
    uint32_t pc, pb, nf, total;
};
template <uint32_t kWaves>
__device__ __forceinline__ RpScan rp_scan(uint32_t cnt, uint32_t byt, uint32_t *s_wc, uint32_t *s_wb, uint32_t lane,
                                          uint32_t wv) {
    uint32_t ic = cnt, ib = byt;                       // inclusive over the wave
#pragma unroll
    for (uint32_t s = 1u; s < 64u; s <<= 1) {
        const uint32_t c2 = __shfl_up(ic, s), b2 = __shfl_up(ib, s);
        if (lane >= s) ic += c2, ib += b2;
    }
    if (lane == 63u) s_wc[wv] = ic, s_wb[wv] = ib;
    __syncthreads();
    RpScan r{ic - cnt, ib - byt, 0u, 0u};
#pragma unroll
    for (uint32_t w = 0; w < kWaves; ++w) {
        if (w < wv) r.pc += s_wc[w], r.pb += s_wb[w];
        r.nf += s_wc[w], r.total += s_wb[w];
    }
    return r;
}

// the frame table (compacted: frame j of the region)
struct RpTable {
    uint64_t src[kRpItems];        // address of the payload's first byte
    uint32_t off[kRpItems];        // the header's offset in the region
    uint32_t len[kRpItems];        // payload bytes
    uint32_t bh[kRpItems];         // b0 | header bytes << 8
};

template <bool kMasked>
__device__ __forceinline__ TmFrame rp_frame(const RpTable &t, uint32_t j, uint32_t key0) {
    TmFrame f;
    f.O = t.off[j];
    f.plen = t.len[j];
    f.hlen = t.bh[j] >> 8;
    f.b0 = t.bh[j] & 0xFFu;
    f.P = f.O + f.hlen;
    f.E = f.P + f.plen;
    f.soff = 0u;
    f.key = kMasked ? FWS_TX_FRAG_KEY(key0, j) : 0u;
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
// Masked: the window is XORed with the key at the window's payload phase before
// it is selected.
template <bool kMasked>
__device__ u32x4 rp_seam_chunk(const RpTable &t, uint32_t nf, uint32_t a, uint32_t j, uint32_t key0) {
    u32x4 x{0u, 0u, 0u, 0u};
    for (; j < nf; ++j) {
        const TmFrame f = rp_frame<kMasked>(t, j, key0);
        if (f.O >= a + 16u) break;
        const uint32_t ho = tm_rel(f.O, a), hp = tm_rel(f.P, a), he = tm_rel(f.E, a);
        if (hp > ho) {                                 // -16 < a - O < 16: the header is 14 bytes at most
            const int off = (int)a - (int)f.O;
            if (off > -16 && off < 16) x = x | tm_and_sel(tm_bytes_at(tm_hdr_vec(f, kMasked), off), ho, hp);
        }
        if (he > hp) {
            const uintptr_t s0 = (uintptr_t)t.src[j], s1 = s0 + f.plen;
            const uintptr_t sa = s0 + (uintptr_t)a - (uintptr_t)f.P;
            const uintptr_t safe = s0 & ~uintptr_t(15);
            uintptr_t b0 = sa & ~uintptr_t(15), b1 = b0 + 16u;
            if (b0 + 16u <= s0 || b0 >= s1) b0 = safe;
            if (b1 + 16u <= s0 || b1 >= s1) b1 = safe;
            u32x4 w = tm_shr_bytes(gload16<false>(b0), gload16<false>(b1), (uint32_t)(sa & 15u));
            if constexpr (kMasked) w = w ^ rotr32(f.key, 8u * ((a - f.P) & 3u));
            x = x | tm_and_sel(w, hp, he);
        }
    }
    return x;
}

// The bytes of the region R, total of them in nf frames (k_tx_multi's mapping: a
// wave's round is one 4 KiB unit, lane chunks 1 KiB apart). A chunk finds its
// frame by rp_frame_of; one inside a single payload is two aligned source loads
// shifted by the source misalignment, any other (a seam: it meets a header or
// the region's end) is built by rp_seam_chunk and stored up to the total.
// Masked: what a full chunk's key needs is known with its addresses, before the
// round's loads are issued -- the frame index, which the seam path keeps anyway,
// and the payload phase (av - P) & 3, two bits a chunk packed into one register
// -- so the eight loads of a thread stay in flight together and the key is
// rotated and XORed into the shifted window on its way to the store. (The
// masked form takes 66 registers against 60 either way; what is done about it
// at 1024 threads is k_reply's launch bound)
template <uint32_t kThreads, bool kMasked>
__device__ __forceinline__ void rp_write_bytes(const RpTable &t, uint32_t nf, uint32_t total, uint8_t *R,
                                               uint32_t lane, uint32_t wv, uint32_t key0) {
    const uint32_t nch = (total + 15u) >> 4;
    const uint32_t lane0 = wv * (64u * kTmU) + lane;
    for (uint32_t r0 = 0; r0 < nch; r0 += kThreads * kTmU) {   // (uniform trip count)
        const uint32_t c0 = r0 + lane0;
        uintptr_t sb[kTmU];
        uint32_t sh[kTmU], fj[kTmU];
        uint32_t full = 0, seam = 0, phases = 0;
#pragma unroll
        for (uint32_t u = 0; u < kTmU; ++u) {
            const uint32_t c = c0 + u * 64u, av = c < nch ? c * 16u : 0u;
            const uint32_t j = nf > 1u ? rp_frame_of(t, nf, av) : 0u;
            fj[u] = j;
            const uint32_t P = t.off[j] + (t.bh[j] >> 8), E = P + t.len[j];
            const bool in = c < nch && av >= P && av + 16u <= E;
            if (in) full |= 1u << u;
            else if (c < nch) seam |= 1u << u;
            const uintptr_t sa = (uintptr_t)t.src[j] + (uintptr_t)(av - P);
            sb[u] = sa & ~uintptr_t(15);
            sh[u] = (uint32_t)(sa & 15u);
            if constexpr (kMasked) phases |= ((av - P) & 3u) << (2u * u);
        }
        u32x4 v0[kTmU], v1[kTmU];
#pragma unroll
        for (uint32_t u = 0; u < kTmU; ++u) {
            if ((full >> u) & 1u) {
                v0[u] = gload16<false>(sb[u]);
                v1[u] = gload16<false>(sh[u] ? sb[u] + 16u : sb[u]);
            } else {
                v0[u] = v1[u] = u32x4{0u, 0u, 0u, 0u};
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < kTmU; ++u)
            if ((full >> u) & 1u) {
                u32x4 w = tm_shr_bytes(v0[u], v1[u], sh[u]);
                if constexpr (kMasked) w = w ^ rotr32(FWS_TX_FRAG_KEY(key0, fj[u]), 8u * ((phases >> (2u * u)) & 3u));
                gstore16<true>((uintptr_t)(R + (c0 + u * 64u) * 16u), w);
            }
        if (seam) {
#pragma unroll
            for (uint32_t u = 0; u < kTmU; ++u) {
                if (!((seam >> u) & 1u)) continue;
                const uint32_t av = (c0 + u * 64u) * 16u;
                tm_store_chunk(R, av, total, rp_seam_chunk<kMasked>(t, nf, av, fj[u], key0));
            }
        }
    }
}

// the records of the first nrec frames
template <uint32_t kThreads, bool kMasked>
__device__ __forceinline__ void rp_put_records(const RpTable &t, uint32_t nrec, fws_frame_info *frames, uint32_t tid,
                                               uint32_t key0) {
    for (uint32_t j = tid; j < nrec; j += kThreads) {
        const TmFrame f = rp_frame<kMasked>(t, j, key0);
        fws_frame_info fi;
        fi.hdr_off = f.O;
        fi.payload_len = f.plen;
        fi.key = f.key;
        fi.opcode = (uint8_t)(f.b0 & 15u);
        fi.fin = (uint8_t)(f.b0 >> 7);
        fi.hdr_len = (uint8_t)f.hlen;
        fi.flags = 0;
        gput(frames + j, fi);
    }
}

}  // namespace fwsk
