// reply_kernels.hip -- fws_gpu_reply_messages_multi: the reply frames of many
// connections built from what a message decode wrote, in one launch, one
// workgroup per read; the link between k_msg_flow / k_msg_multi and k_tx_multi.
//
// A read's items are its n_msgs entries, in order, then the open part: at most
// FWS_MSG_MULTI_MAX_FRAMES + 2. An item gives one frame or none: a PING a PONG,
// a CLOSE a CLOSE (FWS_REPLY_CONTROL, w_socket.h:661-710), a TEXT / BIN entry or
// the open part a data frame (FWS_REPLY_ECHO); nothing follows the CLOSE.
//
// Sequencing. SendFrame's rule (fws_tx_next) over these items is serial in form
// only: every entry ends its message, so after any data frame but the open part
// no message is open, and the one frame whose opcode depends on the connection's
// last_msg_not_fin is the first data frame of the read. So the walk is two
// minima over the items, taken with LDS atomics -- the first CLOSE (items behind
// it are dropped) and the first data item (a continuation when a message is
// open) -- and each item's frame is decided by its own thread.
//
// Frame table. A workgroup scan of (frame?, H(len) + len) over the items gives
// each frame its index and its offset; the frames go, compacted, into an LDS
// table: source address, payload length, offset, b0 and header length. The
// total is known after the scan, before the first store: a refused read
// (invalid, capacity) writes its result and nothing else.
//
// Bytes: the region is written as 16-B chunks from its aligned start, a wave
// taking one 4 KiB unit per round as in k_tx_multi. The frames are irregular, so
// a chunk finds its frame by a binary search in the table's offsets
// (rp_write_bytes, reply_common.h, shared with k_reply_strict as the scan and
// the frame records are). The region's last chunk is stored bytewise up to
// out_len: no byte outside [out_off, out_off + out_len) is written.
//
// kMasked (fws_gpu_reply_messages_multi_client): the frames are client frames,
// masked with FWS_TX_FRAG_KEY(keys[read], frame index); reply_common.h has the
// byte phase. The walk, the refusals and both states are the same. The masked
// instantiations are compiled in a translation unit of their own,
// reply_client_kernels.hip, which includes this file with FWS_REPLY_CLIENT_TU
// defined: instantiated next to the unmasked ones they changed those kernels'
// code (other registers and, at 1024 threads, more instructions; apart, the
// unmasked kernels are instruction for instruction what they were).
#include "fws_device.h"
#include "fws_internal.h"
#include "reply_common.h"
#include "tx_multi_common.h"

#include <type_traits>

namespace fwsk {

struct RpArgs {
    uint8_t *out;
    const uint8_t *dst;
    const uint8_t *ctl;
    const fws_msg_read *reads;
    const fws_msg_info *msgs;
    const fws_msg_result *mres;
    const fws_reply_region *regions;
    fws_frame_info *frames;
    fws_tx_result *res;
    fws_tx_conn *conns;
    fws_reply_state *states;
    uint32_t n_conns;
    uint32_t flags;
};
// the masked form's arguments: RpArgs itself stays what the unmasked kernels take
struct RpArgsMasked {
    RpArgs r;
    const uint32_t *keys;          // one word per read
};

// (the second bound: the masked form takes 66 registers, two over what lets two workgroups of 1024 -- eight waves
// a SIMD -- share a compute unit, so its 1024-thread form is held to 64 at the price of three spilled dwords:
// 512 x 64 KiB 18.2 -> 16.6 us. The 256-thread form measured slower held to 64, and every other instantiation
// gets the default value, its code unchanged)
template <uint32_t kThreads, bool kMasked>
__global__ __launch_bounds__(kThreads, kMasked && kThreads == 1024u ? 8u : kThreads / 256u)
void k_reply(std::conditional_t<kMasked, RpArgsMasked, RpArgs> args) {
    uint32_t key0 = 0u;
    const RpArgs *ap;
    if constexpr (kMasked) ap = &args.r, key0 = args.keys[blockIdx.x];
    else ap = &args;
    const RpArgs &a = *ap;
    constexpr uint32_t kIpt = (kRpItems + kThreads - 1u) / kThreads;   // items per thread, consecutive
    constexpr uint32_t kWaves = kThreads / 64u;
    __shared__ RpTable s_t;
    __shared__ uint32_t s_first_close, s_first_data, s_bad, s_open_item, s_close_code;
    __shared__ uint32_t s_wc[kWaves], s_wb[kWaves];

    const uint32_t tid = threadIdx.x, rd = blockIdx.x;
    const fws_msg_read d = a.reads[rd];                // (uniform addresses: scalar loads)
    const fws_msg_result mr = a.mres[rd];
    const fws_reply_region g = a.regions[rd];
    // Every field used below, in scalar registers here. Left alone the compiler loads a field where it is
    // first used, behind the early exits, one dependent round trip after another (six before the entries'
    // loads, some as vector loads); this empty statement makes them one batch of scalar loads and one wait.
#ifndef FWS_REPLY_NO_HOIST                                // (A/B: make exp EXP_TAG=nohoist EXP_DEFS=-DFWS_REPLY_NO_HOIST)
    asm volatile("" ::"s"(d.dst_off), "s"(d.ctl_off), "s"(d.conn), "s"(d.dst_cap), "s"(d.ctl_cap), "s"(d.msg_base),
                 "s"(d.msg_cap), "s"(mr.status), "s"(mr.n_msgs), "s"(mr.open_opcode), "s"(mr.data_bytes),
                 "s"(mr.ctl_bytes), "s"(mr.open_off), "s"(mr.open_len), "s"(g.out_off), "s"(g.out_cap),
                 "s"(g.frame_base), "s"(g.frame_cap));
#endif

    // ---- what the descriptors alone decide
    if ((g.out_off & 15u) || d.conn >= a.n_conns) {
        if (tid == 0) rp_result(a.res, rd, FWS_ERR_INVALID, 0u, 0u, 0u);
        return;
    }
    fws_tx_conn *const conn = a.conns + d.conn;
    fws_reply_state *const state = a.states + d.conn;
    const bool undelivered = mr.status == FWS_ERR_DECLINED || mr.status == FWS_ERR_INVALID ||
                             mr.n_msgs > d.msg_cap || mr.data_bytes > d.dst_cap || mr.ctl_bytes > d.ctl_cap;
    if (!undelivered && mr.n_msgs > FWS_MSG_MULTI_MAX_FRAMES + 1u) {   // not a decode output
        if (tid == 0) rp_result(a.res, rd, FWS_ERR_INVALID, 0u, 0u, 0u);
        return;
    }
    if (undelivered) {                                 // nothing to answer
        if (tid == 0) rp_result(a.res, rd, 0, 0u, 0u, conn->last_msg_not_fin != 0u ? 1u : 0u);
        return;
    }

    // ---- the items: each thread classifies its own
    // The loads first, so that they are in flight together: every thread's entries, then both states. (The
    // states are read by every wave before thread 0 rewrites them behind the barriers below. Tested where they
    // are loaded, close_sent put the entries' loads, and behind them the payloads', one memory latency later.)
    fws_msg_info e[kIpt];
#pragma unroll
    for (uint32_t k = 0; k < kIpt; ++k) {
        e[k] = fws_msg_info{};
        if (tid * kIpt + k < mr.n_msgs) e[k] = a.msgs[d.msg_base + tid * kIpt + k];
    }
    const uint32_t open = conn->last_msg_not_fin != 0u ? 1u : 0u;
    const uint32_t close_sent = state->close_sent;
    if (tid == 0) {
        s_first_close = kRpNone;
        s_first_data = kRpNone;
        s_bad = 0u;
        s_open_item = 0u;
        s_close_code = 0u;
    }
    __syncthreads();
    const bool control = (a.flags & FWS_REPLY_CONTROL) != 0u, echo = (a.flags & FWS_REPLY_ECHO) != 0u;
    const uint8_t *const dsp = a.dst + d.dst_off, *const csp = a.ctl + d.ctl_off;
    uint32_t kind[kIpt], len[kIpt], op[kIpt];          // kind: 0 no frame, 1 PONG, 2 CLOSE, 3 data entry, 4 the open part
    uint64_t src[kIpt];
#pragma unroll
    for (uint32_t k = 0; k < kIpt; ++k) {
        const uint32_t i = tid * kIpt + k;
        kind[k] = 0u, len[k] = 0u, op[k] = 0u, src[k] = 0u;
        uint64_t ln = 0u;
        if (i < mr.n_msgs) {
            ln = e[k].len;
            op[k] = e[k].opcode;
            if (control && (op[k] == 9u || op[k] == 8u)) {
                kind[k] = op[k] == 9u ? 1u : 2u;
                op[k] = op[k] == 9u ? 10u : 8u;
                src[k] = (uint64_t)(uintptr_t)(csp + e[k].off);
                if (ln > 125u) kind[k] = 0u, atomicOr(&s_bad, 1u);
                else if (kind[k] == 2u) atomicMin(&s_first_close, i);
            } else if (echo && (op[k] == 1u || op[k] == 2u)) {
                kind[k] = 3u;
                src[k] = (uint64_t)(uintptr_t)(dsp + e[k].off);
            }
        } else if (i == mr.n_msgs && echo && mr.open_opcode != 0u && mr.open_len > 0u) {
            kind[k] = 4u;
            ln = mr.open_len;
            op[k] = mr.open_opcode;
            src[k] = (uint64_t)(uintptr_t)(dsp + mr.open_off);
            s_open_item = 1u;
            if (op[k] != 1u && op[k] != 2u) kind[k] = 0u, atomicOr(&s_bad, 1u);
        }
        if (kind[k] >= 3u) {
            if (ln > FWS_MSG_MULTI_MAX_READ) kind[k] = 0u, atomicOr(&s_bad, 1u);   // a read holds no more
            else atomicMin(&s_first_data, i);
        }
        len[k] = (uint32_t)ln;
    }
    __syncthreads();
    if (close_sent != 0u) {                            // nothing more to say
        if (tid == 0) rp_result(a.res, rd, 0, 0u, 0u, open);
        return;
    }
    if (s_bad) {                                       // not a decode output
        if (tid == 0) rp_result(a.res, rd, FWS_ERR_INVALID, 0u, 0u, 0u);
        return;
    }
    const uint32_t fc = s_first_close, fd = s_first_data;

    // ---- frame index and offset: a workgroup scan of (frame?, bytes)
    uint32_t cnt = 0u, byt = 0u;
#pragma unroll
    for (uint32_t k = 0; k < kIpt; ++k) {
        if (tid * kIpt + k > fc) kind[k] = 0u;         // behind the CLOSE
        if (kind[k]) cnt += 1u, byt += tm_hdr_len(len[k], kMasked) + len[k];
    }
    const uint32_t lane = tid & 63u, wv = tid >> 6;
    const RpScan sc = rp_scan<kWaves>(cnt, byt, s_wc, s_wb, lane, wv);
    const uint32_t nf = sc.nf, total = sc.total;
    uint32_t pc = sc.pc, pb = sc.pb;
#pragma unroll
    for (uint32_t k = 0; k < kIpt; ++k) {
        if (!kind[k]) continue;
        const uint32_t i = tid * kIpt + k, hl = tm_hdr_len(len[k], kMasked);
        // fws_tx_next: a data frame that continues an unfinished message is a continuation; FIN but on the open part
        const uint32_t b0 = kind[k] >= 3u ? ((kind[k] == 3u ? 0x80u : 0u) | ((i == fd && open) ? 0u : op[k])) : (0x80u | op[k]);
        s_t.src[pc] = src[k];
        s_t.off[pc] = pb;
        s_t.len[pc] = len[k];
        s_t.bh[pc] = b0 | (hl << 8);
        if (kind[k] == 2u)                             // w_socket.h:668-673
            s_close_code = len[k] >= 2u ? ((uint32_t)gget((const uint8_t *)(uintptr_t)src[k]) << 8) |
                                              gget((const uint8_t *)(uintptr_t)src[k] + 1) : 1005u;
        pc += 1u, pb += hl + len[k];
    }
    __syncthreads();

    // ---- the verdict on the region
    if (total > g.out_cap) {
        if (tid == 0) rp_result(a.res, rd, FWS_ERR_CAPACITY, nf, total, 0u);
        return;
    }

    // ---- the bytes, the frame records
    rp_write_bytes<kThreads, kMasked>(s_t, nf, total, a.out + g.out_off, lane, wv, key0);
    rp_put_records<kThreads, kMasked>(s_t, nf < g.frame_cap ? nf : g.frame_cap, a.frames + g.frame_base, tid, key0);

    // ---- the result and both states, last
    if (tid == 0) {
        // the open part, when it is sent, is the last data frame and leaves its message open; any other ends one
        const uint32_t next_open = fd < fc ? ((s_open_item && fc == kRpNone) ? 1u : 0u) : open;
        rp_result(a.res, rd, 0, nf, total, next_open);
        conn->last_msg_not_fin = next_open;
        conn->frames += nf;
        conn->wire_bytes += total;
        if (fc != kRpNone) {
            state->close_sent = 1u;
            state->close_code = s_close_code;
        }
    }
}

}  // namespace fwsk

using namespace fwsk;

// Two forms by the decode call's max_len, as k_tx_multi: up to 16 KiB 256
// threads, above 1024.
constexpr uint32_t kRpSmallMax = 16u << 10;

#ifndef FWS_REPLY_CLIENT_TU
int fws_launch_reply(const fws_msg_read *reads, uint32_t n, uint32_t max_len, const fws_msg_info *msgs,
                     const uint8_t *dst, const uint8_t *ctl, const fws_msg_result *mres,
                     const fws_reply_region *regions, uint8_t *out, fws_frame_info *frames, fws_tx_result *res,
                     fws_tx_conn *conns, fws_reply_state *states, uint32_t n_conns, uint32_t flags, hipStream_t s) {
    static_assert(sizeof(fws_reply_state) == 16 && sizeof(fws_reply_region) == 32, "the ABI");
    if (!n) return 0;
    RpArgs a{out, dst, ctl, reads, msgs, mres, regions, frames, res, conns, states, n_conns, flags};
    if (max_len <= kRpSmallMax)
        hipLaunchKernelGGL((k_reply<256u, false>), dim3(n), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((k_reply<1024u, false>), dim3(n), dim3(1024), 0, s, a);
    return fws_hip_status(hipGetLastError());
}
#else
int fws_launch_reply_client(const fws_msg_read *reads, uint32_t n, uint32_t max_len, const fws_msg_info *msgs,
                            const uint8_t *dst, const uint8_t *ctl, const fws_msg_result *mres,
                            const fws_reply_region *regions, uint8_t *out, fws_frame_info *frames,
                            fws_tx_result *res, fws_tx_conn *conns, fws_reply_state *states, uint32_t n_conns,
                            uint32_t flags, const uint32_t *keys, hipStream_t s) {
    if (!n) return 0;
    RpArgsMasked a{{out, dst, ctl, reads, msgs, mres, regions, frames, res, conns, states, n_conns, flags}, keys};
    if (max_len <= kRpSmallMax)
        hipLaunchKernelGGL((k_reply<256u, true>), dim3(n), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((k_reply<1024u, true>), dim3(n), dim3(1024), 0, s, a);
    return fws_hip_status(hipGetLastError());
}
#endif
