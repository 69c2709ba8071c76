// publish_kernels.hip -- fws_gpu_publish_messages: messages fanned out to many
// connections in one launch, one workgroup per subscriber; the one-to-many
// counterpart of k_reply (reply_kernels.hip) and k_tx_multi.
//
// A subscriber's items are the fws_join_info records its list names, in list
// order, at most FWS_PUB_MAX_ITEMS of them: one item per thread. The list is an
// array of indices that any number of subscribers may share, and the records
// point into three buffers (dev_dst, dev_store, dev_ctl), so a workgroup's front
// half is two dependent rounds of loads -- every thread its index, then its
// record -- with all threads' loads in flight together, and the connection's two
// state words next to them.
//
// Verdict. Each thread classifies its own record; the flags (invalid, something
// to send, an over-long control frame, a data record over the bound) are ORed
// and the first CLOSE and the first data item are minimised over the wave by
// ballots; lane 0 of each of the four waves that can hold items leaves the
// wave's three words in LDS and every thread reduces them behind one barrier
// (no atomics, so nothing to initialise and no barrier for that). Every record
// is judged, also behind a CLOSE; the refusals are tested in the header's order.
//
// Frame table and bytes: k_reply's. A workgroup scan of (frame?, H(len) + len)
// gives each frame its index and offset, the frames go compacted into the LDS
// table of reply_common.h, and rp_write_bytes / rp_put_records (unmasked) write
// the region and the records. Every frame is whole: FIN = 1 and the record's
// opcode. The total is known before the first store, so a refused subscriber
// writes its result and nothing else.
#include "fws_device.h"
#include "fws_internal.h"
#include "reply_common.h"
#include "tx_multi_common.h"

namespace fwsk {

struct PbArgs {
    uint8_t *out;
    const uint8_t *dst;
    const uint8_t *store;
    const uint8_t *ctl;
    const fws_join_info *msgs;
    const uint32_t *list;
    const fws_pub_sub *subs;
    fws_frame_info *frames;
    fws_tx_result *res;
    fws_tx_conn *conns;
    fws_reply_state *states;
    uint32_t n_msgs, n_list, n_conns, max_len;
};

constexpr uint32_t kPbInvalid = 1u, kPbSome = 2u, kPbControl = 4u, kPbDeclined = 8u;

template <uint32_t kThreads>
__global__ __launch_bounds__(kThreads)
void k_publish(PbArgs a) {
    constexpr uint32_t kWaves = kThreads / 64u, kItemWaves = FWS_PUB_MAX_ITEMS / 64u;   // (items: threads 0 .. 255)
    static_assert(kThreads >= FWS_PUB_MAX_ITEMS && FWS_PUB_MAX_ITEMS <= kRpItems, "one item per thread, one table row");
    __shared__ RpTable s_t;
    __shared__ uint32_t s_wf[kItemWaves], s_wfc[kItemWaves], s_wfd[kItemWaves];
    __shared__ uint32_t s_wc[kWaves], s_wb[kWaves];

    const uint32_t tid = threadIdx.x, sb = blockIdx.x;
    const uint32_t lane = tid & 63u, wv = tid >> 6;
    const fws_pub_sub g = a.subs[sb];                  // (uniform address: scalar loads)
    // one batch of scalar loads and one wait, as in k_reply
    asm volatile("" ::"s"(g.out_off), "s"(g.out_cap), "s"(g.conn), "s"(g.list_off), "s"(g.list_len), "s"(g.frame_base),
                 "s"(g.frame_cap));

    // ---- what the descriptor alone decides
    if ((g.out_off & 15u) || g.conn >= a.n_conns || g.list_len > FWS_PUB_MAX_ITEMS ||
        (uint64_t)g.list_off + g.list_len > a.n_list) {
        if (tid == 0) rp_result(a.res, sb, FWS_ERR_INVALID, 0u, 0u, 0u);
        return;
    }
    fws_tx_conn *const conn = a.conns + g.conn;
    fws_reply_state *const state = a.states + g.conn;

    // ---- the items: each thread loads and classifies its own
    // The index, both states, then the record. (The states are read by every wave here, before thread 0
    // rewrites them behind the barriers below.)
    const bool have = tid < g.list_len;
    uint32_t idx = 0u;
    if (have) idx = a.list[g.list_off + tid];
    const uint32_t open = conn->last_msg_not_fin != 0u ? 1u : 0u;
    const uint32_t close_sent = state->close_sent;
    const bool inr = have && idx < a.n_msgs;
    fws_join_info e{};
    if (inr) e = a.msgs[idx];

    uint32_t kind = 0u, len = 0u, op = 0u, fl = 0u;    // kind: 0 no frame, 1 PING / PONG, 2 CLOSE, 3 data
    uint64_t src = 0u;
    if (have && !inr) fl = kPbInvalid;
    if (inr && e.opcode != 0u && e.where != FWS_JOIN_NOWHERE) {   // anything else is nothing: not judged
        fl = kPbSome;
        op = e.opcode;
        const uint8_t *const b = e.where == FWS_JOIN_IN_DST ? a.dst : (e.where == FWS_JOIN_IN_STORE ? a.store :
                                 (e.where == FWS_JOIN_IN_CTL ? a.ctl : nullptr));
        const bool data = op == 1u || op == 2u, control = op >= 8u && op <= 10u;
        if (!(data || control) || b == nullptr) fl |= kPbInvalid;           // (a where above 3 has no base)
        else if (control) {
            if (e.len > 125u) fl |= kPbControl;
            else kind = op == 8u ? 2u : 1u;
        } else {
            if (e.len > a.max_len || e.len > FWS_TX_MULTI_MAX_SEND) fl |= kPbDeclined;
            else kind = 3u;
        }
        if (kind) {
            len = (uint32_t)e.len;
            src = (uint64_t)(uintptr_t)(b + e.off);
        }
    }
    if (wv < kItemWaves) {   // a wave's verdict by ballots (wave-uniform branch)
        uint32_t wf = 0u;
        if (__ballot(fl & kPbInvalid)) wf |= kPbInvalid;
        if (__ballot(fl & kPbSome)) wf |= kPbSome;
        if (__ballot(fl & kPbControl)) wf |= kPbControl;
        if (__ballot(fl & kPbDeclined)) wf |= kPbDeclined;
        const uint64_t bc = __ballot(kind == 2u), bd = __ballot(kind == 3u);
        if (lane == 0u) {
            s_wf[wv] = wf;
            s_wfc[wv] = bc ? wv * 64u + (uint32_t)__builtin_ctzll(bc) : kRpNone;
            s_wfd[wv] = bd ? wv * 64u + (uint32_t)__builtin_ctzll(bd) : kRpNone;
        }
    }
    __syncthreads();
    uint32_t flags = 0u, fc = kRpNone, fd = kRpNone;
#pragma unroll
    for (uint32_t w = 0; w < kItemWaves; ++w) {
        flags |= s_wf[w];
        fc = s_wfc[w] < fc ? s_wfc[w] : fc;
        fd = s_wfd[w] < fd ? s_wfd[w] : fd;
    }
    int32_t refuse = 0;
    if (flags & kPbInvalid) refuse = FWS_ERR_INVALID;
    else if (close_sent != 0u || !(flags & kPbSome)) {     // nothing more to say, or nothing to say
        if (tid == 0) rp_result(a.res, sb, 0, 0u, 0u, open);
        return;
    } else if (flags & kPbControl) refuse = FWS_ERR_CONTROL_FRAME;
    else if (flags & kPbDeclined) refuse = FWS_ERR_DECLINED;
    else if (open && fd < fc) refuse = FWS_ERR_SEQUENCE;   // a whole message must not be cut into an open one
    if (refuse) {
        if (tid == 0) rp_result(a.res, sb, refuse, 0u, 0u, 0u);
        return;
    }

    // ---- frame index and offset: a workgroup scan of (frame?, bytes)
    if (tid > fc) kind = 0u;                           // behind the CLOSE
    const uint32_t hl = tm_hdr_len(len, false);
    const RpScan sc = rp_scan<kWaves>(kind ? 1u : 0u, kind ? hl + len : 0u, s_wc, s_wb, lane, wv);
    const uint32_t nf = sc.nf, total = sc.total;
    if (kind) {
        s_t.src[sc.pc] = src;
        s_t.off[sc.pc] = sc.pb;
        s_t.len[sc.pc] = len;
        s_t.bh[sc.pc] = 0x80u | op | (hl << 8);
    }
    __syncthreads();

    // ---- the verdict on the region
    if (total > g.out_cap) {
        if (tid == 0) rp_result(a.res, sb, FWS_ERR_CAPACITY, nf, total, 0u);
        return;
    }

    // ---- the bytes, the frame records
    rp_write_bytes<kThreads, false>(s_t, nf, total, a.out + g.out_off, lane, wv, 0u);
    rp_put_records<kThreads, false>(s_t, nf < g.frame_cap ? nf : g.frame_cap, a.frames + g.frame_base, tid, 0u);

    // ---- the result and both states, last
    if (tid == 0) {
        rp_result(a.res, sb, 0, nf, total, open);
        conn->frames += nf;
        conn->wire_bytes += total;
        if (fc != kRpNone) state->close_sent = 1u;
    }
}

}  // namespace fwsk

using namespace fwsk;

// Two forms by max_len, as k_reply: up to 16 KiB 256 threads, above 1024.
constexpr uint32_t kPbSmallMax = 16u << 10;

int fws_launch_publish(const fws_join_info *msgs, uint32_t n_msgs, const uint8_t *dst, const uint8_t *store,
                       const uint8_t *ctl, const uint32_t *list, uint32_t n_list, const fws_pub_sub *subs, uint32_t n,
                       uint32_t max_len, uint8_t *out, fws_frame_info *frames, fws_tx_result *res, fws_tx_conn *conns,
                       fws_reply_state *states, uint32_t n_conns, hipStream_t s) {
    static_assert(sizeof(fws_pub_sub) == 32 && sizeof(fws_join_info) == 32, "the ABI");
    static_assert((uint64_t)FWS_PUB_MAX_ITEMS * (FWS_TX_MULTI_MAX_SEND + 10u) < (1ull << 26), "rp_scan's 32-bit offsets");
    if (!n) return 0;
    PbArgs a{out, dst, store, ctl, msgs, list, subs, frames, res, conns, states, n_msgs, n_list, n_conns, max_len};
    if (max_len <= kPbSmallMax)
        hipLaunchKernelGGL((k_publish<256u>), dim3(n), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((k_publish<1024u>), dim3(n), dim3(1024), 0, s, a);
    return fws_hip_status(hipGetLastError());
}
