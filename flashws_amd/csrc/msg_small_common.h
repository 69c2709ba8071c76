// msg_small_common.h -- what the two per-read message decode kernels share:
// k_msg_multi (msg_multi_kernels.hip, fws_gpu_decode_messages_multi) and
// k_msg_flow (msg_flow_kernels.hip, fws_gpu_decode_messages_flow). Everything
// around wave 0's walk: the descriptor checks, the staging of the read in LDS,
// the gather / unmask / UTF-8 phase over the tables the walk left, the control
// payloads, the entries and the open TEXT part's verdict. The walk, the LDS
// declarations and the state write-back stay with each kernel. k_msg_flow calls
// every function here; k_msg_multi calls ms_refuse and ms_bulk and spells out
// its own checks, staging and write-out, because its 1024-thread form measured
// slower with them called from here: a change to
// ms_check_read, ms_stage, ms_put_entries or ms_open_text goes there too.
//
// The phases run over "elements": the payload pieces of the read in dst / ctl
// order. For k_msg_multi element f is frame f; for k_msg_flow element 0 is the
// lead and frame i is element i + 1.
#pragma once

#include "fws_device.h"
#include "fws_internal.h"

namespace fwsk {

constexpr uint32_t kMsNone = 0xFFFFFFFFu;
constexpr uint32_t kMsFrames = kSmallFrames;
constexpr uint32_t kMsSeeded = 1u << 16;     // region meta: the carried tail is its left context
constexpr uint32_t kMsPrefix = 1u << 17;     // region meta: the open part (errors inside it only)
constexpr uint32_t kMsEntry = 0xFFFFu;       // region meta: its entry

// the LDS tables wave 0 leaves for the workgroup
struct MsTables {
    const uint8_t *sb;             // byte 0 of the staged read
    const uint32_t *po;            // payload start of element f in the read
    const uint32_t *key;
    const uint32_t *dpre;          // data bytes before element f (dst prefix), nel + 1 values
    const uint32_t *cpre;          // control bytes before element f (ctl prefix), nel + 1 values
    const uint32_t *rlo, *rhi;     // TEXT regions of dst, in dst order
    const uint32_t *rmeta;
    uint32_t *rbad;
    uint32_t nel;                  // elements
};

// a read that is not decoded: both results carry the status and nothing else is written
__device__ __forceinline__ void ms_refuse(fws_decode_result *res, fws_msg_result *mres, uint32_t r, int32_t status) {
    fws_decode_result d{};
    d.status = status;
    fws_msg_result m{};
    m.status = status;
    m.err_frame = kMsNone;
    m.open_first_frame = kMsNone;
    gput(res + r, d);
    gput(mres + r, m);
}

// what the descriptor alone decides: 0, or the status to refuse the read with
__device__ __forceinline__ int32_t ms_check_read(const fws_msg_read &d, uint32_t n_conns, uint32_t max_len,
                                                 uint32_t stage) {
    if ((d.wire_off & 15u) || (d.dst_off & 15u) || d.conn >= n_conns) return FWS_ERR_INVALID;
    if (d.len > max_len || d.len > FWS_MSG_MULTI_MAX_READ || d.len > stage) return FWS_ERR_DECLINED;
    return 0;
}

// 1. stage the read's nch chunks behind one zero chunk, two zero chunks behind
// them: all loads of a thread in flight together (decode_small_wg step 1). Clears
// the nbad region verdicts and ends with the barrier. Returns byte 0 of the read:
// a header window at the last offset and a 20-byte payload window that starts up
// to 15 bytes before a payload or ends at the read's end stay in s_buf.
template <uint32_t kChunks, uint32_t kThreads>
__device__ __forceinline__ const uint8_t *ms_stage(u32x4 (&s_buf)[kChunks + 3], uintptr_t base, uint32_t nch,
                                                   uint32_t *s_rbad, uint32_t nbad, uint32_t tid) {
    static_assert(kChunks % (4u * kThreads) == 0, "staging rounds of four loads per thread");
    static_assert(sizeof(s_buf) >= 16u * kChunks + 48u, "one chunk in front of the read, two behind");
#pragma unroll
    for (uint32_t k0 = 0; k0 < kChunks / kThreads; k0 += 4u) {
        u32x4 v0, v1, v2, v3;
        const uint32_t c = tid + k0 * kThreads;
        if (c < nch) v0 = gload16(base + 16u * c);
        if (c + kThreads < nch) v1 = gload16(base + 16u * (c + kThreads));
        if (c + 2u * kThreads < nch) v2 = gload16(base + 16u * (c + 2u * kThreads));
        if (c + 3u * kThreads < nch) v3 = gload16(base + 16u * (c + 3u * kThreads));
        if (c < nch) s_buf[1u + c] = v0;
        if (c + kThreads < nch) s_buf[1u + c + kThreads] = v1;
        if (c + 2u * kThreads < nch) s_buf[1u + c + 2u * kThreads] = v2;
        if (c + 3u * kThreads < nch) s_buf[1u + c + 3u * kThreads] = v3;
    }
    if (tid < 3u) s_buf[tid ? nch + tid : 0u] = u32x4{0u, 0u, 0u, 0u};
    for (uint32_t i = tid; i < nbad; i += kThreads) s_rbad[i] = 0u;
    __syncthreads();
    return (const uint8_t *)(s_buf + 1);
}

// the unmasked byte at dst offset y < db; f: an element at or before its owner
__device__ __forceinline__ uint32_t ms_dst_byte(const MsTables &t, uint32_t y, uint32_t &f) {
    while (t.dpre[f + 1u] <= y) ++f;
    const uint32_t k = y - t.dpre[f];
    return (uint32_t)t.sb[t.po[f] + k] ^ ((t.key[f] >> (8u * (k & 3u))) & 0xFFu);
}

// the owner of dst byte x < db: the last element whose dst prefix is <= x
__device__ __forceinline__ uint32_t ms_owner(const MsTables &t, uint32_t x) {
    uint32_t lo = 0, hi = t.nel - 1u;
    while (lo < hi) {
        const uint32_t m = (lo + hi + 1u) >> 1;
        if (t.dpre[m] <= x) lo = m; else hi = m - 1u;
    }
    return lo;
}

// dst chunk [x0, x0 + 16), zeros from db on: per element that meets it, the 16-B
// source window at the chunk's offset in that element -- five aligned dwords from
// LDS shifted to the source phase; the window may start up to 15 bytes before
// the payload or run past its end, into staged bytes the select drops --, the
// key rotated to the chunk's payload phase, the element's bytes selected.
__device__ __forceinline__ u32x4 ms_dst_chunk(const MsTables &t, uint32_t db, uint32_t x0) {
    u32x4 v{0u, 0u, 0u, 0u};
    if (x0 >= db) return v;
    for (uint32_t f = ms_owner(t, x0); f < t.nel && t.dpre[f] < x0 + 16u; ++f) {
        const uint32_t b = t.dpre[f], e = t.dpre[f + 1u];
        if (e == b) continue;                            // a control frame, an empty fragment, no lead
        const uint32_t k = x0 - b;                       // (mod 2^32 when the element starts inside the chunk)
        const int32_t s = (int32_t)t.po[f] + (int32_t)k; // >= -15
        const uint32_t sh = (uint32_t)s & 3u;
        const uint32_t *w = (const uint32_t *)(t.sb + (s & ~3));
        const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
        const uint32_t rk = rotr32(t.key[f], 8u * (k & 3u));
        v.x |= (__builtin_amdgcn_alignbyte(w1, w0, sh) ^ rk) & sel_bytes(x0, b, e);
        v.y |= (__builtin_amdgcn_alignbyte(w2, w1, sh) ^ rk) & sel_bytes(x0 + 4u, b, e);
        v.z |= (__builtin_amdgcn_alignbyte(w3, w2, sh) ^ rk) & sel_bytes(x0 + 8u, b, e);
        v.w |= (__builtin_amdgcn_alignbyte(w4, w3, sh) ^ rk) & sel_bytes(x0 + 12u, b, e);
    }
    return v;
}

// 3. gather + unmask, 4. UTF-8 on the chunk in registers, then the control
// payloads; by the whole workgroup, when no capacity was exceeded. db data bytes
// go to out, the control payloads to cout. UTF-8 is checked on the bytes as they
// are gathered: the thread that holds a dst chunk takes the dword before it from
// its neighbour lane and tests the chunk once per TEXT region that meets it
// (utf8_err is positional and needs 3 bytes of left context, so chunks are
// independent); a region that fails sets its rbad. Chunks run to db + 3 so an
// unfinished sequence at the end meets zero bytes. A wave takes 64 * steps
// consecutive chunks: the dword before a lane's chunk is its neighbour's last
// (lane 0: lane 63's of the step before; the wave's first chunk: assembled once
// more). old_tail is the left context of a seeded region that starts at dst 0.
template <uint32_t kThreads>
__device__ __forceinline__ void ms_bulk(const MsTables &t, uint32_t db, uint32_t nreg, uint32_t old_tail,
                                        uint8_t *out, uint8_t *cout, uint32_t tid) {
    const uint32_t nck = (db + 18u) >> 4;
    const uint32_t steps = (nck + kThreads - 1u) / kThreads;
    const uint32_t wlane = tid & (kWave - 1u);
    uint32_t carry = 0;
    for (uint32_t st = 0; st < steps; ++st) {            // (the same trips for every lane: the shuffles below)
        const uint32_t c = ((tid / kWave) * steps + st) * kWave + wlane;
        const uint32_t x0 = 16u * c;
        const u32x4 v = c < nck ? ms_dst_chunk(t, db, x0) : u32x4{0u, 0u, 0u, 0u};
        if (c < nck && x0 < db) {
            if (x0 + 16u <= db) {
                gstore16((uintptr_t)out + x0, v);
            } else {                                     // the last chunk: whole dwords, then bytes
                uint32_t j = 0;
                for (; x0 + j + 4u <= db; j += 4u) gput(reinterpret_cast<uint32_t *>(out + x0 + j), v[j >> 2]);
                for (; x0 + j < db; ++j) gput(out + x0 + j, (uint8_t)(v[j >> 2] >> (8u * (j & 3u))));
            }
        }
        if (!nreg) continue;                             // (uniform)
        uint32_t prev = __shfl_up(v.w, 1, kWave);
        if (wlane == 0) prev = carry;
        carry = __shfl(v.w, kWave - 1, kWave);
        if (st == 0) {
            const u32x4 pv = c && c < nck ? ms_dst_chunk(t, db, x0 - 16u) : u32x4{0u, 0u, 0u, 0u};
            if (wlane == 0) prev = pv.w;
        }
        if (c >= nck) continue;
        // ASCII through and through: no region can flag anything here
        if (!((v.x | v.y | v.z | v.w | (c ? prev : old_tail)) & 0x80808080u)) continue;
        // the first region with hi + 3 > x0; the regions that meet the chunk follow it
        uint32_t lo = 0, hi = nreg;
        while (lo < hi) {
            const uint32_t m = (lo + hi) >> 1;
            if (t.rhi[m] + 3u > x0) hi = m; else lo = m + 1u;
        }
        for (uint32_t g = lo; g < nreg && (t.rlo[g] >> 4) <= c; ++g) {
            const uint32_t rl = t.rlo[g], rh = t.rhi[g], meta = t.rmeta[g];
            const uint32_t sx = sel_bytes(x0, rl, rh), sy = sel_bytes(x0 + 4u, rl, rh);
            const uint32_t sz = sel_bytes(x0 + 8u, rl, rh), sw = sel_bytes(x0 + 12u, rl, rh);
            const uint32_t vx = v.x & sx, vy = v.y & sy, vz = v.z & sz, vw = v.w & sw;
            const uint32_t p = c ? prev & sel_bytes(x0 - 4u, rl, rh) : ((meta & kMsSeeded) ? old_tail : 0u);
            if (!((vx | vy | vz | vw | p) & 0x80808080u)) continue;
            uint32_t bad;
            if (meta & kMsPrefix)
                bad = (utf8_err(vx, p) & sx) | (utf8_err(vy, vx) & sy) | (utf8_err(vz, vy) & sz) |
                      (utf8_err(vw, vz) & sw);
            else
                bad = utf8_err(vx, p) | utf8_err(vy, vx) | utf8_err(vz, vy) | utf8_err(vw, vz);
            if (bad) t.rbad[g] = 1u;
        }
    }
    // the control payloads: a wave per element
    for (uint32_t f = tid / kWave; f < t.nel; f += kThreads / kWave) {
        const uint32_t co = t.cpre[f], cl = t.cpre[f + 1u] - co;
        for (uint32_t k = wlane; k < cl; k += kWave)
            gput(cout + co + k, (uint8_t)(t.sb[t.po[f] + k] ^ (uint8_t)(t.key[f] >> (8u * (k & 3u)))));
    }
}

// the ne entries with their verdicts (behind the barrier that ends ms_bulk's
// phase): a TEXT entry is valid when its region saw no error and, where the
// region continues a carried message, that message had none before
template <uint32_t kThreads>
__device__ __forceinline__ void ms_put_entries(const MsTables &t, const fws_msg_info *s_ent, const uint16_t *s_ereg,
                                               uint32_t ne, bool over, uint32_t old_bad, fws_msg_info *msgs,
                                               uint32_t tid) {
    for (uint32_t e = tid; e < ne; e += kThreads) {
        fws_msg_info m = s_ent[e];
        const uint32_t g = s_ereg[e];
        if (!over && g != 0xFFFFu)
            m.utf8_ok = (t.rbad[g] || ((t.rmeta[g] & kMsSeeded) && old_bad)) ? (uint8_t)0 : (uint8_t)1;
        gput(msgs + e, m);
    }
}

// utf8_bad and utf8_tail of an open TEXT part, the last of the nreg regions: the
// verdict so far, and the part's last three bytes (the carried tail shifted on,
// where the part continues it) as the next call's left context
struct MsOpenText {
    uint32_t bad, tail;
};
__device__ __forceinline__ MsOpenText ms_open_text(const MsTables &t, uint32_t nreg, bool open_cont, uint32_t old_tail,
                                                   uint32_t old_bad) {
    const uint32_t g = nreg - 1u, rl = t.rlo[g], rh = t.rhi[g];
    MsOpenText o;
    o.bad = (t.rbad[g] || (open_cont && old_bad)) ? 1u : 0u;
    uint32_t tl = open_cont ? old_tail : 0u;
    uint32_t k = rh - rl > 3u ? rh - 3u : rl;
    if (k < rh) {
        uint32_t f = ms_owner(t, k);
        for (; k < rh; ++k) tl = (tl >> 8) | (ms_dst_byte(t, k, f) << 24);
    }
    o.tail = tl & 0xFFFFFF00u;
    return o;
}

}  // namespace fwsk
