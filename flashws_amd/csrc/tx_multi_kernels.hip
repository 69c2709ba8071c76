// tx_multi_kernels.hip -- fws_gpu_encode_messages_multi: the sends of many
// connections encoded into frames in one launch, one workgroup per send; the
// TX counterpart of k_msg_multi (msg_multi_kernels.hip).
//
// A send is one payload cut into k frames of max_frame payload bytes (the last
// one carries the rest). Every frame but the last has the same size
// S = H(max_frame) + max_frame, H(p) = 2 + 4 masked + (0 | 2 | 8), so frame j
// starts at j S: no scan, no workspace. Opcode and FIN follow SendFrame's rule
// (w_socket.h:845-848, 903-913; fws_tx_next) from the connection's
// last_msg_not_fin in device memory: frame 0 is a continuation when a message
// is open, frames 1.. always are, FIN is `last` on frame k - 1 only; a control
// send is one frame that neither uses nor changes the state.
//
// The verdict of a send (invalid, control frame too long, declined, capacity)
// is a function of its descriptor alone -- the byte count is closed-form -- so
// it is known before the first store, and a refused send writes its result and
// nothing else.
//
// Bytes: the region is written as 16-B chunks from its aligned start, a wave
// taking one 4 KiB unit per round (kTmU chunks per lane). A chunk finds its frame by a
// division (a float reciprocal with a +-1 fix: offsets stay below 2^18). A
// chunk inside one payload is two aligned source loads shifted by the source
// misalignment and XORed with the fragment's key at the frame-relative phase
// (tx_kernels.hip's data path). A chunk that meets a header or the region's end
// (a seam) ORs, for every frame that meets it -- several when max_frame is
// small: three-byte frames put six in one chunk -- the header from registers
// and the keyed source window, each selected on its byte range; the region's
// last chunk is stored bytewise up to out_len. No byte outside
// [out_off, out_off + out_len) is written.
#include "fws_device.h"
#include "fws_internal.h"
#include "tx_multi_common.h"

namespace fwsk {

constexpr uint32_t kTmNoDiv = 1u << 20;      // frame size of a one-frame send: every offset is frame 0's

struct TmArgs {
    uint8_t *out;
    const uint8_t *src;
    const fws_tx_send *sends;
    fws_frame_info *frames;
    fws_tx_result *res;
    fws_tx_conn *conns;
    uint32_t n_conns;
    uint32_t max_len;
};

// the send's frames (wave-uniform)
struct TmPlan {
    uint32_t k;            // frames
    uint32_t m;            // payload bytes of frames 0 .. k - 2
    uint32_t rest;         // payload bytes of frame k - 1
    uint32_t S;            // size of frames 0 .. k - 2 (kTmNoDiv when k == 1)
    float invS;
    uint32_t Hm, Hl;       // header bytes of frames 0 .. k - 2 / of frame k - 1
    uint32_t total;        // bytes of the send
    uint32_t key;          // the send's key
    uint32_t op0;          // opcode of frame 0 (frames 1.. are continuations)
    uint32_t fin;          // FIN of frame k - 1 (the others: 0)
    bool masked;
};

// (TmFrame and the tm_* byte builders: tx_multi_common.h)
__device__ __forceinline__ TmFrame tm_frame(const TmPlan &pl, uint32_t j) {
    const bool lastf = j + 1u >= pl.k;
    TmFrame f;
    f.O = lastf ? (pl.k - 1u) * (pl.k > 1u ? pl.S : 0u) : j * pl.S;
    f.plen = lastf ? pl.rest : pl.m;
    f.hlen = lastf ? pl.Hl : pl.Hm;
    f.P = f.O + f.hlen;
    f.E = f.P + f.plen;
    f.soff = j * pl.m;
    f.key = pl.masked ? FWS_TX_FRAG_KEY(pl.key, j) : 0u;
    f.b0 = ((lastf ? pl.fin : 0u) << 7) | (j == 0u ? pl.op0 : 0u);
    return f;
}

// the frame holding region offset a (< total)
__device__ __forceinline__ uint32_t tm_frame_of(const TmPlan &pl, uint32_t a) {
    uint32_t j = (uint32_t)((float)a * pl.invS);       // a < 2^18: off by one at most
    if (j * pl.S > a) --j;
    else if ((j + 1u) * pl.S <= a) ++j;
    return j < pl.k ? j : pl.k - 1u;
}

// The seam chunk at a: every frame from j on that meets [a, a + 16) gives its
// header bytes and its keyed payload bytes; bytes at or past total stay zero.
// A source block that holds no byte of the frame's payload is replaced by one
// that does (its bytes are never selected), so every load is in bounds.
__device__ u32x4 tm_seam_chunk(const TmPlan &pl, const uint8_t *__restrict__ sp, uint32_t a, uint32_t j) {
    u32x4 x{0u, 0u, 0u, 0u};
    for (; j < pl.k; ++j) {
        const TmFrame f = tm_frame(pl, j);
        if (f.O >= a + 16u) break;
        const uint32_t ho = tm_rel(f.O, a), hp = tm_rel(f.P, a), he = tm_rel(f.E, a);
        if (hp > ho) {                                 // -16 < a - O < 16: the header is 14 bytes at most
            const int off = (int)a - (int)f.O;
            if (off > -16 && off < 16) x = x | tm_and_sel(tm_bytes_at(tm_hdr_vec(f, pl.masked), off), ho, hp);
        }
        if (he > hp) {
            // the source byte of region offset o is at SX + o
            const uintptr_t s0 = (uintptr_t)(sp + f.soff), s1 = s0 + f.plen;
            const uintptr_t sa = s0 + (uintptr_t)a - (uintptr_t)f.P;
            const uintptr_t safe = s0 & ~uintptr_t(15);
            uintptr_t b0 = sa & ~uintptr_t(15), b1 = b0 + 16u;
            if (b0 + 16u <= s0 || b0 >= s1) b0 = safe;
            if (b1 + 16u <= s0 || b1 >= s1) b1 = safe;
            const uint32_t rk = rotr32(f.key, 8u * ((a - f.P) & 3u));
            const u32x4 w = tm_shr_bytes(gload16<false>(b0), gload16<false>(b1), (uint32_t)(sa & 15u)) ^ rk;
            x = x | tm_and_sel(w, hp, he);
        }
    }
    return x;
}

__device__ __forceinline__ void tm_result(const TmArgs &a, uint32_t s, int32_t status, uint32_t n_frames,
                                          uint64_t out_len, uint32_t lmnf) {
    fws_tx_result r{};
    r.status = status;
    r.n_frames = n_frames;
    r.out_len = out_len;
    r.last_msg_not_fin = lmnf;
    gput(a.res + s, r);
}

template <uint32_t kThreads>
__global__ __launch_bounds__(kThreads) void k_tx_multi(TmArgs a) {
    const uint32_t tid = threadIdx.x, sd = blockIdx.x;
    const fws_tx_send d = a.sends[sd];                 // (a uniform address: scalar loads)

    // ---- the verdict, from the descriptor alone
    const uint32_t ft = d.frame_type;
    const bool control = (ft & 8u) != 0;
    int32_t status = 0;
    if ((d.out_off & 15u) || d.conn >= a.n_conns || !(ft == 1u || ft == 2u || (ft >= 8u && ft <= 10u)))
        status = FWS_ERR_INVALID;
    else if (control && d.len > 125u)
        status = FWS_ERR_CONTROL_FRAME;
    else if (d.len > a.max_len || d.len > FWS_TX_MULTI_MAX_SEND)
        status = FWS_ERR_DECLINED;
    if (status) {
        if (tid == 0) tm_result(a, sd, status, 0u, 0u, 0u);
        return;
    }
    TmPlan pl;
    pl.masked = d.masked != 0;
    const bool one = control || d.max_frame == 0u || d.len <= d.max_frame;
    pl.k = one ? 1u : d.len / d.max_frame + (d.len % d.max_frame != 0u ? 1u : 0u);
    if (pl.k > FWS_TX_MULTI_MAX_FRAMES) {
        if (tid == 0) tm_result(a, sd, FWS_ERR_DECLINED, 0u, 0u, 0u);
        return;
    }
    pl.m = one ? d.len : d.max_frame;
    pl.rest = d.len - (pl.k - 1u) * pl.m;
    pl.Hm = tm_hdr_len(pl.m, pl.masked);
    pl.Hl = tm_hdr_len(pl.rest, pl.masked);
    pl.S = one ? kTmNoDiv : pl.Hm + pl.m;
    pl.invS = 1.0f / (float)pl.S;
    pl.total = (pl.k - 1u) * (pl.Hm + pl.m) + pl.Hl + pl.rest;   // <= 128 KiB + 256 * 14
    pl.key = d.key;
    if (pl.total > d.out_cap) {
        if (tid == 0) tm_result(a, sd, FWS_ERR_CAPACITY, pl.k, pl.total, 0u);
        return;
    }

    // ---- sequencing: the connection's state is read by every wave before thread 0 rewrites it
    fws_tx_conn *const conn = a.conns + d.conn;
    const uint32_t open = conn->last_msg_not_fin != 0u ? 1u : 0u;
    const uint32_t lastb = d.last != 0 ? 1u : 0u;
    pl.op0 = (open && !control) ? 0u : ft;
    pl.fin = lastb;
    const uint32_t next_open = control ? open : (lastb ? 0u : 1u);
    __syncthreads();

    uint8_t *const R = a.out + d.out_off;
    const uint8_t *const sp = a.src + d.src_off;
    const uint32_t total = pl.total, nch = (total + 15u) >> 4;

    // ---- the bytes
    // a wave's round is one 4 KiB unit, lane chunks 1 KiB apart (tx_kernels.hip's
    // tx_unit): frame seams, at least max_frame bytes apart, spread over the waves.
    // (Chunks t, t + T, ... put the seams of 4 KiB frames into a few waves, four to
    // a round, built one after another: 64 x 64 KiB in 4 KiB frames took 14.8 us,
    // 8.4 with this mapping)
    const uint32_t lane0 = (tid >> 6) * (64u * kTmU) + (tid & 63u);
    for (uint32_t r0 = 0; r0 < nch; r0 += kThreads * kTmU) {   // (uniform trip count)
        const uint32_t c0 = r0 + lane0;
        uintptr_t sb[kTmU];
        uint32_t sh[kTmU], rk[kTmU], fj[kTmU];
        uint32_t full = 0, seam = 0;
#pragma unroll
        for (uint32_t u = 0; u < kTmU; ++u) {
            const uint32_t c = c0 + u * 64u, av = c < nch ? c * 16u : 0u;
            const uint32_t j = tm_frame_of(pl, av);
            const TmFrame f = tm_frame(pl, j);
            fj[u] = j;
            const bool in = c < nch && av >= f.P && av + 16u <= f.E;
            if (in) full |= 1u << u;
            else if (c < nch) seam |= 1u << u;
            const uintptr_t sa = (uintptr_t)(sp + f.soff) + (uintptr_t)(av - f.P);
            sb[u] = sa & ~uintptr_t(15);
            sh[u] = (uint32_t)(sa & 15u);
            rk[u] = rotr32(f.key, 8u * ((av - f.P) & 3u));
        }
        u32x4 v0[kTmU], v1[kTmU];
#pragma unroll
        for (uint32_t u = 0; u < kTmU; ++u) {
            if ((full >> u) & 1u) {
                // default-policy loads: the second block of lane L is the first of lane L + 1
                v0[u] = gload16<false>(sb[u]);
                v1[u] = gload16<false>(sh[u] ? sb[u] + 16u : sb[u]);
            } else {
                v0[u] = v1[u] = u32x4{0u, 0u, 0u, 0u};
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < kTmU; ++u)
            if ((full >> u) & 1u)
                gstore16<true>((uintptr_t)(R + (c0 + u * 64u) * 16u), tm_shr_bytes(v0[u], v1[u], sh[u]) ^ rk[u]);
        if (seam) {
#pragma unroll
            for (uint32_t u = 0; u < kTmU; ++u) {
                if (!((seam >> u) & 1u)) continue;
                const uint32_t av = (c0 + u * 64u) * 16u;
                tm_store_chunk(R, av, total, tm_seam_chunk(pl, sp, av, fj[u]));
            }
        }
    }

    // ---- the frame records
    const uint32_t nrec = pl.k < d.frame_cap ? pl.k : d.frame_cap;
    for (uint32_t j = tid; j < nrec; j += kThreads) {
        const TmFrame f = tm_frame(pl, j);
        fws_frame_info fi;
        fi.hdr_off = f.O;
        fi.payload_len = f.plen;
        fi.key = f.key;
        fi.opcode = (uint8_t)(f.b0 & 15u);
        fi.fin = (uint8_t)(f.b0 >> 7);
        fi.hdr_len = (uint8_t)f.hlen;
        fi.flags = 0;
        gput(a.frames + d.frame_base + j, fi);
    }

    // ---- the result and the connection's state
    if (tid == 0) {
        tm_result(a, sd, 0, pl.k, total, next_open);
        conn->last_msg_not_fin = next_open;
        conn->frames += pl.k;
        conn->wire_bytes += total;
    }
}

}  // namespace fwsk

using namespace fwsk;

// Two forms, chosen by the caller's bound on a send as in k_msg_multi: up to
// 16 KiB (<= 1024 + a few chunks) 256 threads, several workgroups to a compute
// unit; above, 1024 threads, so that a 128 KiB send is 8 chunks per thread
// (measured, DESIGN.md 4.6.1: a 64 KiB send takes 10.9 us at 256 threads and 7.7
// at 1024; up to 16 KiB the small form is level or ahead).
constexpr uint32_t kTmSmallMax = 16u << 10;

// tuning hook (tools/msg_bench.py --tx-multi measures both forms on every
// shape): 0 = by max_len (the default), 256 / 1024 = that form for every call
static int g_tm_threads = 0;
extern "C" __attribute__((visibility("default"))) int fws_internal_set_tx_multi_threads(int threads) {
    const int old = g_tm_threads;
    g_tm_threads = threads == 256 || threads == 1024 ? threads : 0;
    return old;
}

int fws_launch_tx_multi(uint8_t *out, const uint8_t *src, const fws_tx_send *sends, uint32_t n, uint32_t max_len,
                        fws_frame_info *frames, fws_tx_result *res, fws_tx_conn *conns, uint32_t n_conns,
                        hipStream_t s) {
    static_assert(sizeof(fws_tx_conn) == 32 && sizeof(fws_tx_send) == 64 && sizeof(fws_tx_result) == 32, "the ABI");
    static_assert(FWS_TX_MULTI_MAX_SEND + FWS_TX_MULTI_MAX_FRAMES * 14u < (1u << 18), "tm_frame_of's float quotient");
    if (!n) return 0;
    TmArgs a{out, src, sends, frames, res, conns, n_conns, max_len};
    if (g_tm_threads ? g_tm_threads == 256 : max_len <= kTmSmallMax)
        hipLaunchKernelGGL((k_tx_multi<256u>), dim3(n), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((k_tx_multi<1024u>), dim3(n), dim3(1024), 0, s, a);
    return fws_hip_status(hipGetLastError());
}
