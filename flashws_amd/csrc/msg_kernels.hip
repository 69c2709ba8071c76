// msg_kernels.hip -- the message planner of fws_gpu_decode_messages: from the
// decoded frame list to messages (RFC 6455 §5.4 fragmentation, §5.5 control
// frames), on the device.
//
// k_msg_plan: one thread per frame, a block scan and a decoupled look-back (the
// protocol of plan_common.h -- epoch-tagged words, the workgroup order of
// plan_block_order -- with 8 tagged words per workgroup instead of one) over a
// 56-byte state, MsgScan, whose combine is associative:
//   - sums: data frames, data bytes, control bytes, completed entries;
//   - the last message-start frame (TEXT / BIN) and the data bytes / frames
//     since it (the right operand's when it holds a start, else the left's
//     plus the right's sums), so the frame that completes a message knows its
//     first frame, length and dst offset without reading another workgroup's
//     frames;
//   - whether the last data frame left a message open (the right operand's when
//     it holds a data frame) and what the segment's first data frame expects
//     (a continuation: open; a start: closed);
//   - the first sequencing error: the operands' own, or the right operand's
//     first data frame when its expectation does not meet the left's state.
// The stream starts closed: workgroup 0's exclusive prefix is a data-bearing,
// closed state. Every thread writes exactly one fws_frame_desc: a data frame
// before the first error its payload region at its data rank, every other
// thread (later data frames, control frames, indices past the frame count) a
// zero-length region -- the data ranks first, the rest from the back of the
// cap slots -- so the gather runs over cap descriptors, a count the host knows.
// The thread of the first error, or else of the last frame, writes the result.
//
// fws_gpu_decode_messages_carry (MsgPlanArgs.carry != null): the initial state
// comes from the connection's fws_msg_carry -- closed, or open with its opcode
// and no start frame in this call (start = kMsNoStart) -- wherever the closed
// state stands otherwise; a truncated data frame is an absent element; the
// result's resume_off never goes back; and the result's thread leaves the next
// carry, but for its UTF-8 fields, in fws_msg_carry_next for k_utf8_msgs.
//
// k_msg_ctl: the control payloads (<= 125 B each), one wave per control frame.
#include "fws_device.h"
#include "fws_internal.h"
#include "plan_common.h"

namespace fwsk {

constexpr uint32_t kMsData = 1u;        // the segment holds a data frame
constexpr uint32_t kMsOpen = 2u;        // its last data frame leaves a message open
constexpr uint32_t kMsStart = 4u;       // it holds a message-start frame (start, sb, sf, opcode)
constexpr uint32_t kMsFirstCont = 8u;   // its first data frame is a continuation
constexpr uint32_t kMsOpShift = 8;      // opcode of the last start frame
constexpr uint32_t kMsOpMask = 0xFu << kMsOpShift;
constexpr uint32_t kMsNoStart = 0xFFFFFFFFu;   // MsgScan.start: the open message began in an earlier call

struct MsgScan {
    uint64_t db;        // data bytes
    uint64_t cb;        // control bytes
    uint64_t sb;        // data bytes since (and of) the last start frame; no start: db
    uint32_t nd;        // data frames
    uint32_t ne;        // completed entries
    uint32_t sf;        // data frames since the last start frame; no start: nd
    uint32_t start;     // the last start frame
    uint32_t err;       // first sequencing error, or 0xFFFFFFFF
    uint32_t fd;        // first data frame, or 0xFFFFFFFF
    uint32_t fl;        // kMs*
    uint32_t pad;
};
static_assert(sizeof(MsgScan) == 56, "14 dwords");
constexpr int kMsDwords = 14;

__device__ __forceinline__ MsgScan ms_identity() {
    MsgScan o{};
    o.err = 0xFFFFFFFFu;
    o.fd = 0xFFFFFFFFu;
    return o;
}

__device__ __forceinline__ MsgScan ms_combine(const MsgScan &L, const MsgScan &R) {
    MsgScan o;
    o.db = L.db + R.db;
    o.cb = L.cb + R.cb;
    o.nd = L.nd + R.nd;
    o.ne = L.ne + R.ne;
    const bool rs = (R.fl & kMsStart) != 0, rd = (R.fl & kMsData) != 0, ld = (L.fl & kMsData) != 0;
    o.sb = rs ? R.sb : L.sb + R.sb;
    o.sf = rs ? R.sf : L.sf + R.sf;
    o.start = rs ? R.start : L.start;
    o.fd = L.fd < R.fd ? L.fd : R.fd;                  // (the initial state bears data but no frame)
    o.fl = ((rs ? R.fl : L.fl) & (kMsStart | kMsOpMask)) | ((rd ? R.fl : L.fl) & kMsOpen) |
           ((ld ? L.fl : R.fl) & kMsFirstCont) | ((L.fl | R.fl) & kMsData);
    uint32_t e = L.err < R.err ? L.err : R.err;
    if (ld && rd && ((L.fl & kMsOpen) != 0) != ((R.fl & kMsFirstCont) != 0) && R.fd < e) e = R.fd;
    o.err = e;
    o.pad = 0;
    return o;
}

__device__ __forceinline__ MsgScan ms_shfl_up(const MsgScan &v, int o) {
    uint32_t w[kMsDwords];
    __builtin_memcpy(w, &v, sizeof(MsgScan));
#pragma unroll
    for (int i = 0; i < kMsDwords; ++i) w[i] = __shfl_up(w[i], o, kWave);
    MsgScan r;
    __builtin_memcpy(&r, w, sizeof(MsgScan));
    return r;
}
__device__ __forceinline__ MsgScan ms_shfl_down(const MsgScan &v, int o) {
    uint32_t w[kMsDwords];
    __builtin_memcpy(w, &v, sizeof(MsgScan));
#pragma unroll
    for (int i = 0; i < kMsDwords; ++i) w[i] = __shfl_down(w[i], o, kWave);
    MsgScan r;
    __builtin_memcpy(&r, w, sizeof(MsgScan));
    return r;
}

// Look-back payloads: 8 words per workgroup and kind (aggregate, inclusive
// prefix), each word 48 value bits under the call's 16-bit epoch tag -- the
// one-word protocol of plan_common.h widened: a word that carries the tag was
// written by this call (each is written once per call), so a reader needs no
// fence and no flag, only all 8 tags; words of earlier calls are ignored.
// Byte counts fit 48 bits (the resolve refuses streams of 2^39 bytes and up).
constexpr int kMsSlot = 8;
constexpr uint64_t kMsVal = (1ull << 48) - 1;
__device__ __forceinline__ void ms_publish(uint64_t *slot, const MsgScan &v, uint64_t tag) {
    lb_store(slot + 0, tag | (v.db & kMsVal));
    lb_store(slot + 1, tag | (v.cb & kMsVal));
    lb_store(slot + 2, tag | (v.sb & kMsVal));
    lb_store(slot + 3, tag | v.nd | ((uint64_t)(v.fl & 0xFFFFu) << 32));
    lb_store(slot + 4, tag | v.ne | ((uint64_t)(v.fd & 0xFFFFu) << 32));
    lb_store(slot + 5, tag | v.sf | ((uint64_t)(v.fd >> 16) << 32));
    lb_store(slot + 6, tag | v.start);
    lb_store(slot + 7, tag | v.err);
}
__device__ __forceinline__ bool ms_fetch(const uint64_t *slot, uint64_t tag, MsgScan &r) {
    uint64_t q[kMsSlot];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < kMsSlot; ++i) q[i] = lb_load(slot + i);
#pragma unroll
    for (int i = 0; i < kMsSlot; ++i) ok = ok && (q[i] & ~kMsVal) == tag;
    r.db = q[0] & kMsVal;
    r.cb = q[1] & kMsVal;
    r.sb = q[2] & kMsVal;
    r.nd = (uint32_t)q[3];
    r.fl = (uint32_t)(q[3] >> 32) & 0xFFFFu;
    r.ne = (uint32_t)q[4];
    r.sf = (uint32_t)q[5];
    r.fd = ((uint32_t)(q[4] >> 32) & 0xFFFFu) | (((uint32_t)(q[5] >> 32) & 0xFFFFu) << 16);
    r.start = (uint32_t)q[6];
    r.err = (uint32_t)q[7];
    r.pad = 0;
    return ok;
}

struct MsgPlanArgs {
    const fws_frame_info *frames;
    const uint32_t *n_dev;          // device frame count (<= cap)
    const fws_decode_result *res;   // the parse's result
    uint64_t len;                   // stream bytes
    uint32_t cap, msg_cap;
    uint64_t dst_cap, ctl_cap;
    fws_frame_desc *descs;          // [cap]
    uint64_t *ctl_off;              // [cap]
    fws_msg_info *msgs;             // [msg_cap]
    fws_msg_result *out;
    uint64_t *agg, *pre;            // look-back words, kMsSlot per workgroup
    uint32_t *ticket;
    uint32_t epoch;
    const fws_msg_carry *carry;     // null: the stream starts closed (fws_gpu_decode_messages)
    fws_msg_carry_next *cnext;      // with carry: the next carry, for k_utf8_msgs
};

// The state before frame 0: data-bearing and closed, or what the carry holds.
__device__ __forceinline__ MsgScan ms_init(const MsgPlanArgs &a) {
    MsgScan init = ms_identity();
    init.fl = kMsData;
    if (a.carry) {
        // a start of its own (no bytes, no frames yet): an identity combined on its
        // left -- the look-back's lanes past the stop -- must not take its place
        init.fl |= kMsStart;
        init.start = kMsNoStart;
        const uint32_t op = a.carry->open_opcode & 0xFu;
        if (op) init.fl |= kMsOpen | (op << kMsOpShift);
    }
    return init;
}

// The exclusive prefix of workgroup blk (its aggregate is `agg`), by wave 0:
// 64 earlier workgroups per round, nearest first, up to the nearest inclusive
// prefix; the position before workgroup 0 is the initial state.
__device__ __forceinline__ MsgScan ms_lookback(const MsgPlanArgs &a, uint32_t blk, const MsgScan &agg, int lane) {
    const uint64_t tag = (uint64_t)a.epoch << 48;
    const MsgScan init = ms_init(a);
    if (blk == 0) {
        if (lane == 0) ms_publish(a.pre, ms_combine(init, agg), tag);
        return init;
    }
    if (lane == 0) ms_publish(a.agg + (uint64_t)blk * kMsSlot, agg, tag);
    MsgScan acc = ms_identity();
    for (int64_t j = (int64_t)blk - 1;; j -= kWave) {
        const int64_t idx = j - lane;
        MsgScan v = init;                              // before workgroup 0: the initial state
        bool is_pre = true;
        if (idx >= 0) {
            for (;;) {
                if (ms_fetch(a.pre + (uint64_t)idx * kMsSlot, tag, v)) break;
                if (ms_fetch(a.agg + (uint64_t)idx * kMsSlot, tag, v)) {
                    is_pre = false;
                    break;
                }
            }
        }
        const uint64_t pm = __ballot(is_pre);
        const int stop = pm ? __builtin_ctzll(pm) : kWave;
        if (lane > stop) v = ms_identity();
        // lane L holds workgroup j - L: lane 0 <- v[63] . ... . v[1] . v[0]
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const MsgScan t = ms_shfl_down(v, o);
            if (lane + o < kWave) v = ms_combine(t, v);
        }
        MsgScan v0;
        {
            uint32_t w[kMsDwords];
            __builtin_memcpy(w, &v, sizeof(MsgScan));
#pragma unroll
            for (int i = 0; i < kMsDwords; ++i) w[i] = __builtin_amdgcn_readfirstlane(w[i]);
            __builtin_memcpy(&v0, w, sizeof(MsgScan));
        }
        acc = ms_combine(v0, acc);
        if (stop < kWave) break;
    }
    if (lane == 0) ms_publish(a.pre + (uint64_t)blk * kMsSlot, ms_combine(acc, agg), tag);
    return acc;
}

__global__ __launch_bounds__(kBlock) void k_msg_plan(MsgPlanArgs a) {
    __shared__ MsgScan s_w[kBlock / kWave];
    __shared__ MsgScan s_bp;
    const uint32_t blk = plan_block_order(a.ticket);
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    uint32_t n = *a.n_dev;
    if (n > a.cap) n = a.cap;
    const uint64_t i64 = (uint64_t)blk * kBlock + threadIdx.x;
    const uint32_t i = (uint32_t)i64;
    const bool has = i64 < n;
    fws_frame_info fi{};
    if (has) fi = a.frames[i];
    const uint64_t po = fi.hdr_off + fi.hdr_len;
    const bool trunc = (fi.flags & FWS_FRAME_TRUNCATED) != 0 || po + fi.payload_len > a.len;
    uint64_t present = fi.payload_len;
    if (trunc) present = a.len > po ? a.len - po : 0;
    const bool cm = a.carry != nullptr;                // whole frames only: a truncated data frame is absent
    const bool data = has && fi.opcode <= 2u && !(cm && trunc), ctl = has && fi.opcode >= 8u;
    const bool ctl_bad = ctl && (!fi.fin || fi.payload_len > 125u);
    const bool ctl_ok = ctl && !ctl_bad && !trunc;
    const bool done = data && fi.fin && !trunc;

    MsgScan el = ms_identity();
    if (data) {
        el.db = el.sb = present;
        el.nd = el.sf = 1u;
        el.ne = done ? 1u : 0u;
        el.fd = i;
        el.fl = kMsData | (done ? 0u : kMsOpen);
        if (fi.opcode) {
            el.fl |= kMsStart | ((uint32_t)fi.opcode << kMsOpShift);
            el.start = i;
        } else {
            el.fl |= kMsFirstCont;
        }
    } else if (ctl_bad) {
        el.err = i;
    } else if (ctl_ok) {
        el.cb = fi.payload_len;
        el.ne = 1u;
    }

    // block scan: inclusive in the wave, the waves' aggregates through LDS
    MsgScan inc = el;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const MsgScan t = ms_shfl_up(inc, o);
        if (lane >= o) inc = ms_combine(t, inc);
    }
    if (lane == kWave - 1) s_w[w] = inc;
    MsgScan ex = ms_shfl_up(inc, 1);
    if (lane == 0) ex = ms_identity();
    __syncthreads();
    MsgScan before = ms_identity(), agg = ms_identity();
#pragma unroll
    for (int k = 0; k < kBlock / kWave; ++k) {
        const MsgScan sk = s_w[k];
        if (k < w) before = ms_combine(before, sk);
        agg = ms_combine(agg, sk);
    }
    ex = ms_combine(before, ex);
    if (w == 0) {
        const MsgScan bp = ms_lookback(a, blk, agg, lane);
        if (lane == 0) s_bp = bp;
    }
    __syncthreads();
    ex = ms_combine(s_bp, ex);                         // the state before frame i
    const MsgScan in = ms_combine(ex, el);             // and after it
    const bool good = has && in.err == 0xFFFFFFFFu;    // frame i and all before it are in sequence

    if (i64 < a.cap) {
        fws_frame_desc d{0, 0, 0u, 0u};
        uint32_t slot;
        if (data) {
            slot = ex.nd;
            if (good) d = fws_frame_desc{po, present, fi.key, 0u};
        } else {
            slot = a.cap - 1u - (i - ex.nd);
        }
        a.descs[slot] = d;
        a.ctl_off[i] = good && ctl_ok ? ex.cb : ~0ull;
    }
    if (good && (done || ctl_ok) && ex.ne < a.msg_cap) {
        fws_msg_info m{};
        if (ctl_ok) {
            m.off = ex.cb;
            m.len = fi.payload_len;
            m.first_frame = i;
            m.n_data_frames = 1u;
            m.opcode = fi.opcode;
        } else {
            const bool st = fi.opcode != 0;
            m.len = (st ? 0 : ex.sb) + present;
            m.off = in.db - m.len;
            m.first_frame = st ? i : ex.start;
            if (cm && !st && ex.start == kMsNoStart) {   // began in an earlier call: this call's part
                m.first_frame = ex.fd != 0xFFFFFFFFu ? ex.fd : i;
                m.flags = FWS_MSG_CONTINUED;
            }
            m.n_data_frames = (st ? 0u : ex.sf) + 1u;
            m.opcode = st ? fi.opcode : (uint8_t)((ex.fl & kMsOpMask) >> kMsOpShift);
        }
        m.last_frame = i;
        a.msgs[ex.ne] = m;
    }

    // the result: the state before the first error, or after the last frame
    const bool first_err = has && in.err == i && ex.err == 0xFFFFFFFFu;
    const bool last_ok = has && i == n - 1u && good;
    if (first_err || last_ok || (n == 0 && i64 == 0)) {
        const MsgScan &S = first_err ? ex : in;
        const bool open = (has || cm) && (S.fl & kMsOpen) != 0;
        const bool cont = cm && open && S.start == kMsNoStart;   // the carried message is still open
        fws_msg_result r{};
        r.n_msgs = S.ne;
        r.err_frame = first_err ? i : 0xFFFFFFFFu;
        r.open_first_frame = open ? (cont ? S.fd : S.start) : 0xFFFFFFFFu;
        r.open_opcode = open ? (S.fl & kMsOpMask) >> kMsOpShift : 0u;
        r.n_data_frames = S.nd;
        r.data_bytes = S.db;
        r.ctl_bytes = S.cb;
        r.open_off = open ? S.db - S.sb : 0;
        r.open_len = open ? S.sb : 0;
        uint64_t end = po + fi.payload_len;            // the end of the last frame processed
        if (end > a.len) end = a.len;
        if (first_err || ((ctl || cm) && trunc)) end = fi.hdr_off;
        if (!has) end = 0;
        const int32_t parse = a.res->status;
        const bool over = S.ne > a.msg_cap || S.db > a.dst_cap || S.cb > a.ctl_cap;
        if (cm) {
            // parts are delivered, never resubmitted; nothing is when a byte / entry
            // capacity was exceeded: the same bytes come again, the carry stays
            r.resume_off = over ? 0 : end;
            const fws_msg_carry old = *a.carry;
            fws_msg_carry_next c{};
            c.next.open_opcode = r.open_opcode;
            c.next.open_frames = open ? (cont ? old.open_frames : 0u) + S.sf : 0u;
            c.next.open_bytes = open ? (cont ? old.open_bytes : 0) + S.sb : 0;
            c.next.prev_open_opcode = old.open_opcode;
            c.next.prev_open_frames = old.open_frames;
            c.next.prev_open_bytes = old.open_bytes;
            c.next.wire_bytes = old.wire_bytes + end;
            c.next.n_msgs = old.n_msgs + S.ne;
            c.deny = over ? 1u : 0u;
            c.open_cont = cont ? 1u : 0u;
            c.old_tail = old.utf8_tail;
            c.old_bad = old.utf8_bad;
            *a.cnext = c;
        } else {
            r.resume_off = open ? a.frames[S.start].hdr_off : end;
        }
        r.status = first_err ? (ctl_bad ? FWS_ERR_CONTROL_FRAME : FWS_ERR_SEQUENCE)
                             : (parse != 0 ? parse : (over ? FWS_ERR_CAPACITY : 0));
        *a.out = r;
    }
}

// One wave per control frame listed by the planner (ctl_off[i] != ~0): its
// payload, unmasked, to ctl + ctl_off[i]. Waves take 64 frames at a time.
__global__ __launch_bounds__(kBlock) void k_msg_ctl(const uint8_t *__restrict__ wire,
                                                    const fws_frame_info *__restrict__ frames,
                                                    const uint32_t *__restrict__ n_dev, uint32_t cap,
                                                    const uint64_t *__restrict__ ctl_off,
                                                    const fws_msg_result *__restrict__ res, uint64_t ctl_cap,
                                                    uint8_t *__restrict__ ctl, const uint32_t *__restrict__ deny) {
    uint32_t n = *n_dev;
    if (n > cap) n = cap;
    if (res->ctl_bytes > ctl_cap) return;              // nothing is written when they do not fit
    if (deny && *deny) return;                         // (the carry form: nor when anything else does not)
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t nw = (uint64_t)gridDim.x * (kBlock / kWave);
    for (uint64_t b = ((uint64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave) * kWave; b < n; b += nw * kWave) {
        const uint64_t i = b + (uint64_t)lane;
        const uint64_t off = i < n ? ctl_off[i] : ~0ull;
        for (uint64_t m = __ballot(off != ~0ull); m; m &= m - 1u) {
            const int L = __builtin_ctzll(m);
            const uint64_t o = readlane64(off, L);
            const fws_frame_info fi = frames[b + (uint64_t)L];
            const uint64_t po = fi.hdr_off + fi.hdr_len;
            for (uint32_t k = (uint32_t)lane; k < fi.payload_len; k += kWave)
                ctl[o + k] = (uint8_t)(wire[po + k] ^ (uint8_t)(fi.key >> (8u * (k & 3u))));
        }
    }
}

}  // namespace fwsk

using namespace fwsk;

int fws_launch_msg_plan(fws_gpu_ctx *ctx, uint64_t len, const fws_frame_info *frames, uint32_t cap,
                        const uint32_t *n_dev, const fws_decode_result *res, fws_msg_info *msgs, uint32_t msg_cap,
                        uint64_t dst_cap, uint64_t ctl_cap, fws_msg_result *out, bool reset, hipStream_t s,
                        const fws_msg_carry *carry) {
    fws_plan_ws &ws = ctx->plan;
    const uint64_t nb = cap ? ((uint64_t)cap + kBlock - 1) / kBlock : 1;
    if (cap > ctx->msg.cap) return FWS_ERR_CAPACITY;
    int r = fws_plan_next_epoch(ws, s);
    if (r) return r;
    // no word of an old call may carry this call's tag: zero them when the epochs
    // restarted since this context's last plan (a wrap, a regrown plan workspace),
    // and for a call whose launches are replayed with one epoch
    const bool restarted = ws.epoch <= ctx->msg.last_epoch;
    ctx->msg.last_epoch = ws.epoch;
    if (reset || restarted) {
        const size_t bytes = (size_t)(ctx->msg.cap / kBlock + 2) * kMsSlot * 8;
        if ((r = fws_hip_status(hipMemsetAsync(ctx->msg.agg, 0, bytes, s)))) return r;
        if ((r = fws_hip_status(hipMemsetAsync(ctx->msg.pre, 0, bytes, s)))) return r;
    }
    MsgPlanArgs a;
    a.frames = frames;
    a.n_dev = n_dev;
    a.res = res;
    a.len = len;
    a.cap = cap;
    a.msg_cap = msg_cap;
    a.dst_cap = dst_cap;
    a.ctl_cap = ctl_cap;
    a.descs = ctx->msg.descs;
    a.ctl_off = ctx->msg.ctl_off;
    a.msgs = msgs;
    a.out = out;
    a.agg = ctx->msg.agg;
    a.pre = ctx->msg.pre;
    a.ticket = ws.ticket;
    a.epoch = ws.epoch;
    a.carry = carry;
    a.cnext = ctx->msg.cnext;
    hipLaunchKernelGGL(k_msg_plan, dim3((unsigned)nb), dim3(kBlock), 0, s, a);
    return fws_hip_status(hipGetLastError());
}

int fws_launch_msg_ctl(fws_gpu_ctx *ctx, const uint8_t *wire, const fws_frame_info *frames, uint32_t cap,
                       const uint32_t *n_dev, const fws_msg_result *res, uint8_t *ctl, uint64_t ctl_cap,
                       hipStream_t s, const uint32_t *deny) {
    if (cap == 0) return 0;
    uint64_t blocks = ((uint64_t)cap + kBlock - 1) / kBlock;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(k_msg_ctl, dim3((unsigned)blocks), dim3(kBlock), 0, s, wire, frames, n_dev, cap,
                       ctx->msg.ctl_off, res, ctl_cap, ctl, deny);
    return fws_hip_status(hipGetLastError());
}
