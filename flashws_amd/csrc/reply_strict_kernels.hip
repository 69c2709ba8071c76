// reply_strict_kernels.hip -- fws_gpu_reply_messages_strict: k_reply
// (reply_kernels.hip) for a server that fails a connection on the device (RFC
// 6455 §7.1.7): the read's first failing item is answered with a CLOSE frame
// that carries the status code and nothing follows it.
//
// A read's items are its n_msgs entries, the open part and, last, the decode's
// error. Each item's thread computes the item's failure code from the entry,
// the decode's result and the connection's decode state (fws_msg_carry or
// fws_msg_flow, read only); index << 16 | code goes into a third LDS minimum
// beside k_reply's first CLOSE and first data item, so the minimum is the first
// failing item and its code at once. A CLOSE entry's own code and reason are
// judged by one wave behind the first barrier -- only the read's first CLOSE:
// the wave of the thread that holds it takes the reason as zero-padded dwords,
// four bytes a lane, and runs the UTF-8 step of fws_device.h over them (left
// context zero, the zeros behind the end close a cut sequence). No byte outside
// [2, len) of the payload is loaded.
//
// With a failing item f at or before the first CLOSE answered, item f becomes a
// CLOSE frame of two payload bytes whose table source is kRsCodes below, the
// items behind it give no frame, and the scan, the table and the byte phases
// run as in k_reply (reply_common.h). The array is one aligned 16-byte block,
// so the seam path's "block that holds a byte of the payload" is the array.
//
// kMasked (fws_gpu_reply_messages_strict_client): client frames as in k_reply;
// the failing CLOSE is a frame like any other, counted in the key's frame index:
// 8 bytes, its two code bytes masked. As there, the masked instantiations are
// compiled apart: reply_strict_client_kernels.hip includes this file with
// FWS_REPLY_CLIENT_TU defined.
#include "fws_device.h"
#include "fws_internal.h"
#include "reply_common.h"
#include "tx_multi_common.h"

#include <type_traits>

namespace fwsk {

// big-endian 1002, 1007, 1009: the payloads of the failing CLOSE
__device__ __attribute__((aligned(16))) const uint8_t kRsCodes[16] = {0x03, 0xEA, 0x03, 0xEF, 0x03, 0xF1};

constexpr uint32_t kRsItems = kRpItems + 1u;             // and the decode's error

struct RsArgs {
    uint8_t *out;
    const uint8_t *dst;
    const uint8_t *ctl;
    const fws_msg_read *reads;
    const fws_msg_info *msgs;
    const fws_msg_result *mres;
    const uint8_t *cstates;        // fws_msg_carry (stride 64) or fws_msg_flow (stride 96)
    const fws_reply_region *regions;
    fws_frame_info *frames;
    fws_tx_result *res;
    fws_tx_conn *conns;
    fws_reply_state *states;
    uint64_t limit;                // max_message_bytes, 0: none
    uint32_t stride;
    uint32_t n_conns;
    uint32_t flags;
};
struct RsArgsMasked {              // (as RpArgsMasked: RsArgs itself stays what the unmasked kernels take)
    RsArgs r;
    const uint32_t *keys;          // one word per read
};

__device__ __forceinline__ uint32_t rs_code_src(uint32_t code) {   // offset in kRsCodes
    return code == 1002u ? 0u : (code == 1007u ? 2u : 4u);
}

// RFC 6455 §7.4 and the IANA registry: 1000-1003, 1007-1014, 3000-4999 may appear in a CLOSE frame
__device__ __forceinline__ bool rs_code_valid(uint32_t c) {
    return (c >= 1000u && c <= 1003u) || (c >= 1007u && c <= 1014u) || (c >= 3000u && c <= 4999u);
}

// The failure code of a CLOSE payload [p, p + n), n <= 125 and uniform, by the whole wave (0: none)
__device__ __forceinline__ uint32_t rs_close_code(const uint8_t *p, uint32_t n, uint32_t lane) {
    if (n <= 1u) return n ? 1002u : 0u;
    const uint32_t code = ((uint32_t)gget(p) << 8) | gget(p + 1);
    uint32_t x = 0u;                                   // reason bytes [4 lane, 4 lane + 4), zero past the end
#pragma unroll
    for (uint32_t b = 0; b < 4u; ++b) {
        const uint32_t j = 2u + 4u * lane + b;
        if (j < n) x |= (uint32_t)gget(p + j) << (8u * b);
    }
    uint32_t prev = __shfl_up(x, 1);
    if (lane == 0u) prev = 0u;
    // 123 bytes end in dword 30: dword 31 and lanes 32.. see only the zeros that close a cut sequence
    const bool bad = __ballot(utf8_err(x, prev) != 0u) != 0ull;
    return !rs_code_valid(code) ? 1002u : (bad ? 1007u : 0u);
}

template <uint32_t kThreads, bool kMasked>
__global__ __launch_bounds__(kThreads) void k_reply_strict(std::conditional_t<kMasked, RsArgsMasked, RsArgs> args) {
    uint32_t key0 = 0u;
    const RsArgs *ap;
    if constexpr (kMasked) ap = &args.r, key0 = args.keys[blockIdx.x];
    else ap = &args;
    const RsArgs &a = *ap;
    constexpr uint32_t kIpt = (kRsItems + kThreads - 1u) / kThreads;   // items per thread, consecutive
    constexpr uint32_t kWaves = kThreads / 64u;
    __shared__ RpTable s_t;
    __shared__ uint32_t s_first_close, s_first_data, s_bad, s_open_item, s_close_code;
    __shared__ uint32_t s_any_close, s_fail;           // the first CLOSE entry whatever the flags; index << 16 | code
    __shared__ uint32_t s_wc[kWaves], s_wb[kWaves];

    const uint32_t tid = threadIdx.x, rd = blockIdx.x;
    const fws_msg_read d = a.reads[rd];                // (uniform addresses: scalar loads)
    const fws_msg_result mr = a.mres[rd];
    const fws_reply_region g = a.regions[rd];
    // one batch of scalar loads and one wait, as in k_reply
    asm volatile("" ::"s"(d.dst_off), "s"(d.ctl_off), "s"(d.conn), "s"(d.dst_cap), "s"(d.ctl_cap), "s"(d.msg_base),
                 "s"(d.msg_cap), "s"(mr.status), "s"(mr.n_msgs), "s"(mr.open_opcode), "s"(mr.data_bytes),
                 "s"(mr.ctl_bytes), "s"(mr.open_off), "s"(mr.open_len), "s"(g.out_off), "s"(g.out_cap),
                 "s"(g.frame_base), "s"(g.frame_cap));

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
    // The loads first, in flight together: every thread's entries, both states and the decode's state.
    fws_msg_info e[kIpt];
#pragma unroll
    for (uint32_t k = 0; k < kIpt; ++k) {
        e[k] = fws_msg_info{};
        if (tid * kIpt + k < mr.n_msgs) e[k] = a.msgs[d.msg_base + tid * kIpt + k];
    }
    const uint32_t open = conn->last_msg_not_fin != 0u ? 1u : 0u;
    const uint32_t close_sent = state->close_sent;
    // The decode's state is not written while this kernel runs: its dwords are scalar loads like the descriptors,
    // in flight with the entries' loads. (As loads through the struct pointer they came out as vector loads from
    // a uniform address, issued by every wave of every workgroup: DESIGN.md 4.6.3 has the A/B.)
    typedef const __attribute__((address_space(4))) uint32_t c_u32;
    const c_u32 *const cw = (const c_u32 *)(uintptr_t)(a.cstates + (uint64_t)d.conn * a.stride);
    static_assert(offsetof(fws_msg_carry, open_bytes) == 8 && offsetof(fws_msg_carry, utf8_bad) == 20 &&
                  offsetof(fws_msg_carry, prev_open_bytes) == 32 && offsetof(fws_msg_flow, frame_unread) == 64, "dwords");
    const uint64_t c_open_bytes = cw[2] | ((uint64_t)cw[3] << 32), c_prev_bytes = cw[8] | ((uint64_t)cw[9] << 32);
    const uint32_t c_utf8_bad = cw[5];
    const uint64_t c_unread = a.stride == sizeof(fws_msg_flow) ? cw[16] | ((uint64_t)cw[17] << 32) : 0u;
    if (tid == 0) {
        s_first_close = kRpNone;
        s_first_data = kRpNone;
        s_bad = 0u;
        s_open_item = 0u;
        s_close_code = kRpNone;
        s_any_close = kRpNone;
        s_fail = kRpNone;
    }
    __syncthreads();
    const bool control = (a.flags & FWS_REPLY_CONTROL) != 0u, echo = (a.flags & FWS_REPLY_ECHO) != 0u;
    const uint8_t *const dsp = a.dst + d.dst_off, *const csp = a.ctl + d.ctl_off;
    const uint64_t limit = a.limit;
    // kind: 0 no frame, 1 PONG, 2 CLOSE, 3 data entry, 4 the open part, 5 the failing CLOSE
    uint32_t kind[kIpt], len[kIpt], op[kIpt];
    uint64_t src[kIpt];
#pragma unroll
    for (uint32_t k = 0; k < kIpt; ++k) {
        const uint32_t i = tid * kIpt + k;
        kind[k] = 0u, len[k] = 0u, op[k] = 0u, src[k] = 0u;
        uint64_t ln = 0u;
        uint32_t code = 0u;
        if (i < mr.n_msgs) {
            ln = e[k].len;
            op[k] = e[k].opcode;
            if (op[k] == 9u || op[k] == 8u) {
                src[k] = (uint64_t)(uintptr_t)(csp + e[k].off);
                if (op[k] == 8u && ln <= 125u) atomicMin(&s_any_close, i);   // judged below
                if (control) {
                    kind[k] = op[k] == 9u ? 1u : 2u;
                    if (ln > 125u) kind[k] = 0u, atomicOr(&s_bad, 1u);
                    else if (kind[k] == 2u) atomicMin(&s_first_close, i);
                }
            } else if (op[k] == 1u || op[k] == 2u) {
                const uint64_t before = (e[k].flags & FWS_MSG_CONTINUED) ? c_prev_bytes : 0u;
                if (limit != 0u && (ln > limit || before > limit - ln)) code = 1009u;
                else if (op[k] == 1u && e[k].utf8_ok == 0u) code = 1007u;
                if (echo) {
                    kind[k] = 3u;
                    src[k] = (uint64_t)(uintptr_t)(dsp + e[k].off);
                }
            }
        } else if (i == mr.n_msgs) {                   // the open part, judged even when it is empty
            if (limit != 0u && (c_open_bytes > limit || c_unread > limit - c_open_bytes)) code = 1009u;
            else if (mr.open_opcode == 1u && c_utf8_bad != 0u) code = 1007u;
            if (echo && mr.open_opcode != 0u && mr.open_len > 0u) {
                kind[k] = 4u;
                ln = mr.open_len;
                op[k] = mr.open_opcode;
                src[k] = (uint64_t)(uintptr_t)(dsp + mr.open_off);
                s_open_item = 1u;
                if (op[k] != 1u && op[k] != 2u) kind[k] = 0u, atomicOr(&s_bad, 1u);
            }
        } else if (i == mr.n_msgs + 1u) {              // the decode's error
            const int32_t st = mr.status;
            if (st == FWS_ERR_TOO_LARGE) code = 1009u;
            else if (st == FWS_ERR_RSV || st == FWS_ERR_NOT_MASKED || st == FWS_ERR_MASKED || st == FWS_ERR_OPCODE ||
                     st == FWS_ERR_CONTROL_FRAME || st == FWS_ERR_SEQUENCE)
                code = 1002u;
        }
        if (kind[k] == 3u || kind[k] == 4u) {
            if (ln > FWS_MSG_MULTI_MAX_READ) kind[k] = 0u, atomicOr(&s_bad, 1u);   // a read holds no more
            else atomicMin(&s_first_data, i);
        }
        if (code) atomicMin(&s_fail, (i << 16) | code);
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
    const uint32_t lane = tid & 63u, wv = tid >> 6;

    // ---- the first CLOSE entry's code and reason, by the wave of the thread that holds it
    const uint32_t ac = s_any_close;                   // (uniform: a read without a CLOSE skips this and its barrier)
    if (ac != kRpNone && ((ac / kIpt) >> 6) == wv) {
        uint32_t lo = 0u, hi = 0u, cl = 0u;
#pragma unroll
        for (uint32_t k = 0; k < kIpt; ++k)
            if (tid * kIpt + k == ac) lo = (uint32_t)src[k], hi = (uint32_t)(src[k] >> 32), cl = len[k];
        const uint32_t owner = (ac / kIpt) & 63u;
        lo = __shfl(lo, owner), hi = __shfl(hi, owner), cl = __shfl(cl, owner);
        const uint32_t code = rs_close_code((const uint8_t *)(uintptr_t)(((uint64_t)hi << 32) | lo), cl, lane);
        if (code && lane == 0u) atomicMin(&s_fail, (ac << 16) | code);
    }
    if (ac != kRpNone) __syncthreads();
    const uint32_t fc = s_first_close, fd = s_first_data, ff = s_fail;
    // a CLOSE answered before the first failing item ends the read as in k_reply
    const bool failing = ff != kRpNone && (ff >> 16) <= fc;
    const uint32_t cut = failing ? ff >> 16 : fc, fail_code = ff & 0xFFFFu;

    // ---- frame index and offset: a workgroup scan of (frame?, bytes)
    uint32_t cnt = 0u, byt = 0u;
#pragma unroll
    for (uint32_t k = 0; k < kIpt; ++k) {
        const uint32_t i = tid * kIpt + k;
        if (i > cut) kind[k] = 0u;                     // behind the CLOSE, echoed or failing
        if (failing && i == cut) kind[k] = 5u, len[k] = 2u;
        if (kind[k]) cnt += 1u, byt += tm_hdr_len(len[k], kMasked) + len[k];
    }
    const RpScan sc = rp_scan<kWaves>(cnt, byt, s_wc, s_wb, lane, wv);
    const uint32_t nf = sc.nf, total = sc.total;
    uint32_t pc = sc.pc, pb = sc.pb;
#pragma unroll
    for (uint32_t k = 0; k < kIpt; ++k) {
        if (!kind[k]) continue;
        const uint32_t i = tid * kIpt + k, hl = tm_hdr_len(len[k], kMasked);
        const bool data = kind[k] == 3u || kind[k] == 4u;
        // fws_tx_next: a data frame that continues an unfinished message is a continuation; FIN but on the open part
        const uint32_t b0 = data ? ((kind[k] == 3u ? 0x80u : 0u) | ((i == fd && open) ? 0u : op[k]))
                                 : (0x80u | (kind[k] == 1u ? 10u : 8u));
        const bool was_close = i < mr.n_msgs && op[k] == 8u;
        if (kind[k] == 2u || (kind[k] == 5u && was_close))   // the code received (w_socket.h:668-673)
            s_close_code = e[k].len >= 2u ? ((uint32_t)gget((const uint8_t *)(uintptr_t)src[k]) << 8) |
                                                gget((const uint8_t *)(uintptr_t)src[k] + 1) : 1005u;
        if (pc < kRpItems) {                           // (259 frames are refused below)
            s_t.src[pc] = kind[k] == 5u ? (uint64_t)(uintptr_t)(kRsCodes + rs_code_src(fail_code)) : src[k];
            s_t.off[pc] = pb;
            s_t.len[pc] = len[k];
            s_t.bh[pc] = b0 | (hl << 8);
        }
        pc += 1u, pb += hl + len[k];
    }
    __syncthreads();

    // ---- the verdict on the region
    if (nf > kRpItems) {                               // 257 entries, an open part and an error: not a decode output
        if (tid == 0) rp_result(a.res, rd, FWS_ERR_INVALID, 0u, 0u, 0u);
        return;
    }
    if (total > g.out_cap) {
        if (tid == 0) rp_result(a.res, rd, FWS_ERR_CAPACITY, nf, total, 0u);
        return;
    }

    // ---- the bytes, the frame records
    rp_write_bytes<kThreads, kMasked>(s_t, nf, total, a.out + g.out_off, lane, wv, key0);
    rp_put_records<kThreads, kMasked>(s_t, nf < g.frame_cap ? nf : g.frame_cap, a.frames + g.frame_base, tid, key0);

    // ---- the result and both states, last
    if (tid == 0) {
        // data frames lie before the cut; the open part, when it is sent, is the last one and leaves its message open
        const uint32_t next_open = fd < cut ? ((s_open_item && mr.n_msgs < cut) ? 1u : 0u) : open;
        rp_result(a.res, rd, 0, nf, total, next_open);
        conn->last_msg_not_fin = next_open;
        conn->frames += nf;
        conn->wire_bytes += total;
        if (cut != kRpNone) {
            state->close_sent = 1u;
            if (s_close_code != kRpNone) state->close_code = s_close_code;
            if (failing) state->fail_code = fail_code;
        }
    }
}

}  // namespace fwsk

using namespace fwsk;

// Two forms by the decode call's max_len, as k_reply: up to 16 KiB 256 threads, above 1024.
constexpr uint32_t kRsSmallMax = 16u << 10;

#ifndef FWS_REPLY_CLIENT_TU
int fws_launch_reply_strict(const fws_msg_read *reads, uint32_t n, uint32_t max_len, const fws_msg_info *msgs,
                            const uint8_t *dst, const uint8_t *ctl, const fws_msg_result *mres,
                            const uint8_t *conn_states, uint32_t conn_state_stride, uint64_t max_message_bytes,
                            const fws_reply_region *regions, uint8_t *out, fws_frame_info *frames, fws_tx_result *res,
                            fws_tx_conn *conns, fws_reply_state *states, uint32_t n_conns, uint32_t flags,
                            hipStream_t s) {
    static_assert(sizeof(fws_reply_state) == 16 && offsetof(fws_reply_state, fail_code) == 8, "the ABI");
    static_assert(sizeof(fws_msg_carry) == 64 && sizeof(fws_msg_flow) == 96 && offsetof(fws_msg_flow, frame_unread) == 64,
                  "the decode states");
    if (!n) return 0;
    RsArgs a{out, dst, ctl, reads, msgs, mres, conn_states, regions, frames, res, conns, states, max_message_bytes,
             conn_state_stride, n_conns, flags};
    if (max_len <= kRsSmallMax)
        hipLaunchKernelGGL((k_reply_strict<256u, false>), dim3(n), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((k_reply_strict<1024u, false>), dim3(n), dim3(1024), 0, s, a);
    return fws_hip_status(hipGetLastError());
}
#else
int fws_launch_reply_strict_client(const fws_msg_read *reads, uint32_t n, uint32_t max_len, const fws_msg_info *msgs,
                                   const uint8_t *dst, const uint8_t *ctl, const fws_msg_result *mres,
                                   const uint8_t *conn_states, uint32_t conn_state_stride,
                                   uint64_t max_message_bytes, const fws_reply_region *regions, uint8_t *out,
                                   fws_frame_info *frames, fws_tx_result *res, fws_tx_conn *conns,
                                   fws_reply_state *states, uint32_t n_conns, uint32_t flags, const uint32_t *keys,
                                   hipStream_t s) {
    if (!n) return 0;
    RsArgsMasked a{{out, dst, ctl, reads, msgs, mres, conn_states, regions, frames, res, conns, states,
                    max_message_bytes, conn_state_stride, n_conns, flags}, keys};
    if (max_len <= kRsSmallMax)
        hipLaunchKernelGGL((k_reply_strict<256u, true>), dim3(n), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((k_reply_strict<1024u, true>), dim3(n), dim3(1024), 0, s, a);
    return fws_hip_status(hipGetLastError());
}
#endif
