// join_kernels.hip -- fws_gpu_join_messages: the messages of many connections
// that arrive over several reads put together on the device, one workgroup per
// read; a sibling of k_reply (reply_kernels.hip) that reads what a message
// decode wrote and changes nothing in it.
//
// A read's items are its n_msgs entries, in order, then the open part: at most
// FWS_MSG_MULTI_MAX_FRAMES + 2. Every entry gets a record that says where the
// whole message lies. A control entry and a data message that is whole in this
// read stay where the decode put them; nothing is copied. The parts of a
// message that spans reads are appended, read by read, to one half of the
// connection's slot of dev_store, and the record of the FWS_MSG_CONTINUED entry
// that completes it points there.
//
// Serial in form only. A read has at most one CONTINUED entry, which is its
// first data entry, and at most one open part, so what depends on the
// connection's state is two appends at most: the continued part, then the open
// part. Every thread classifies its own entries; two minima and a count, taken
// with LDS atomics, find the CONTINUED entry and say whether decode and join
// are in step. The verdict is known behind one barrier, before the first global
// store: a refused read writes its result and nothing else.
//
// Ping-pong. The half toggles when a joined message is delivered, so the
// message delivered by this read stays intact while the read's open part starts
// the next one in the other half.
//
// Bytes. An append's destination is slot + half * H + fill, any address, so the
// copy works in 16-B chunks aligned to the destination: a chunk is two aligned
// source loads shifted by the source's misalignment against it (tm_shr_bytes),
// the partial first and last chunks are stored bytewise, and no byte outside
// the appended range is written. A source block that holds no byte of the part
// is replaced by one that does (its bytes are never selected), so the loads
// touch only blocks of dev_dst that hold a byte of the part. Every offset is 64
// bits wide: conn * store_stride passes 4 GiB.
#include "fws_device.h"
#include "fws_internal.h"
#include "tx_multi_common.h"

namespace fwsk {

constexpr uint32_t kJnItems = FWS_MSG_MULTI_MAX_FRAMES + 1u;   // the entries: a lead's and one per header
constexpr uint32_t kJnNone = 0xFFFFFFFFu;

struct JnArgs {
    uint8_t *store;
    const uint8_t *dst;
    const fws_msg_read *reads;
    const fws_msg_info *msgs;
    const fws_msg_result *mres;
    fws_join_info *joined;
    fws_join_result *res;
    fws_join_state *states;
    uint64_t stride;
    uint32_t n_conns;
};

__device__ __forceinline__ void jn_result(fws_join_result *res, uint32_t r, int32_t status, uint32_t n_joined,
                                          uint64_t copied, uint32_t open_opcode, uint32_t dropped) {
    fws_join_result x{};
    x.status = status;
    x.n_joined = n_joined;
    x.copied = copied;
    x.open_opcode = open_opcode;
    x.dropped = dropped;
    gput(res + r, x);
}

// one append that copies: len bytes (> 0) from src to dst, both any address
struct JnJob {
    uintptr_t src, dst;
    uint32_t len;
};

// bytes [lo, hi) (offsets 0..16) of x to the chunk at A
__device__ __forceinline__ void jn_store_bytes(uintptr_t A, uint32_t lo, uint32_t hi, const u32x4 &x) {
    const uint32_t xw[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (uint32_t i = 0; i < 16u; ++i)                 // (static indices: no scratch)
        if (i >= lo && i < hi) gput((uint8_t *)(A + i), (uint8_t)(xw[i >> 2] >> (8u * (i & 3u))));
}

// The destination's chunks, kTmU to a thread per round, the loads of a round in
// flight together. Chunk c lies at A = (dst & ~15) + 16 c and takes the source
// bytes from sa = src + (A - dst) on, which for the first chunk may lie up to 15
// bytes in front of src: those bytes are not selected.
template <uint32_t kThreads>
__device__ __forceinline__ void jn_copy(const JnJob &j, uint32_t tid) {
    const uintptr_t s0 = j.src, s1 = j.src + j.len, t0 = j.dst, t1 = j.dst + j.len;
    const uintptr_t tb = t0 & ~uintptr_t(15), safe = s0 & ~uintptr_t(15);
    const uint32_t nch = (uint32_t)((t1 + 15u - tb) >> 4);
    for (uint32_t r0 = 0; r0 < nch; r0 += kThreads * kTmU) {   // (uniform trip count)
        u32x4 v0[kTmU], v1[kTmU];
        uint32_t sh[kTmU];
#pragma unroll
        for (uint32_t u = 0; u < kTmU; ++u) {
            const uint32_t c = r0 + u * kThreads + tid;
            v0[u] = v1[u] = u32x4{0u, 0u, 0u, 0u};
            sh[u] = 0u;
            if (c >= nch) continue;
            const uintptr_t sa = s0 + (tb + 16u * (uintptr_t)c) - t0;   // (mod 2^64: tb <= t0)
            uintptr_t b0 = sa & ~uintptr_t(15), b1 = b0 + 16u;
            sh[u] = (uint32_t)(sa & 15u);
            if (b0 + 16u <= s0 || b0 >= s1) b0 = safe;
            if (sh[u] == 0u || b1 + 16u <= s0 || b1 >= s1) b1 = b0;
            v0[u] = gload16<false>(b0);
            v1[u] = gload16<false>(b1);
        }
#pragma unroll
        for (uint32_t u = 0; u < kTmU; ++u) {
            const uint32_t c = r0 + u * kThreads + tid;
            if (c >= nch) continue;
            const uintptr_t A = tb + 16u * (uintptr_t)c;
            const u32x4 w = tm_shr_bytes(v0[u], v1[u], sh[u]);
            if (A >= t0 && A + 16u <= t1) gstore16<false>(A, w);
            else jn_store_bytes(A, A < t0 ? (uint32_t)(t0 - A) : 0u, A + 16u > t1 ? (uint32_t)(t1 - A) : 16u, w);
        }
    }
}

template <uint32_t kThreads>
__global__ __launch_bounds__(kThreads)
void k_join(JnArgs a) {
    constexpr uint32_t kIpt = (kJnItems + kThreads - 1u) / kThreads;   // entries per thread, consecutive
    __shared__ uint32_t s_first_data, s_cont, s_ncont, s_bad, s_cont_len;

    const uint32_t tid = threadIdx.x, rd = blockIdx.x;
    const fws_msg_read d = a.reads[rd];                // (uniform addresses: scalar loads)
    const fws_msg_result mr = a.mres[rd];
    // every field used below in one batch of scalar loads and one wait (k_reply's hoist)
    asm volatile("" ::"s"(d.dst_off), "s"(d.ctl_off), "s"(d.conn), "s"(d.dst_cap), "s"(d.ctl_cap), "s"(d.msg_base),
                 "s"(d.msg_cap), "s"(mr.status), "s"(mr.n_msgs), "s"(mr.open_opcode), "s"(mr.data_bytes),
                 "s"(mr.ctl_bytes), "s"(mr.open_off), "s"(mr.open_len));

    // ---- what the descriptors alone decide
    if (d.conn >= a.n_conns) {
        if (tid == 0) jn_result(a.res, rd, FWS_ERR_INVALID, 0u, 0u, 0u, 0u);
        return;
    }
    fws_join_state *const state = a.states + d.conn;
    const fws_join_state S = *state;                   // (read by every wave before thread 0 rewrites it, last)
    const bool undelivered = mr.status == FWS_ERR_DECLINED || mr.status == FWS_ERR_INVALID ||
                             mr.n_msgs > d.msg_cap || mr.data_bytes > d.dst_cap || mr.ctl_bytes > d.ctl_cap;
    if (undelivered) {                                 // nothing to join
        if (tid == 0) jn_result(a.res, rd, 0, 0u, 0u, S.open_opcode, S.dropped);
        return;
    }
    if (mr.n_msgs > kJnItems) {                        // not a decode output
        if (tid == 0) jn_result(a.res, rd, FWS_ERR_INVALID, 0u, 0u, 0u, 0u);
        return;
    }

    // ---- the entries: each thread classifies its own
    fws_msg_info e[kIpt];
#pragma unroll
    for (uint32_t k = 0; k < kIpt; ++k) {
        e[k] = fws_msg_info{};
        if (tid * kIpt + k < mr.n_msgs) e[k] = a.msgs[d.msg_base + tid * kIpt + k];
    }
    if (tid == 0) {
        s_first_data = kJnNone;
        s_cont = kJnNone;
        s_ncont = 0u;
        s_bad = 0u;
        s_cont_len = 0u;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kIpt; ++k) {
        const uint32_t i = tid * kIpt + k;
        if (i >= mr.n_msgs || e[k].opcode >= 8u) continue;
        atomicMin(&s_first_data, i);
        if (e[k].len > FWS_MSG_MULTI_MAX_READ) atomicOr(&s_bad, 1u);   // a read holds no more
        else if (e[k].flags & FWS_MSG_CONTINUED) {
            atomicMin(&s_cont, i);
            atomicAdd(&s_ncont, 1u);
            s_cont_len = (uint32_t)e[k].len;           // (used only when there is one such entry)
        }
    }
    __syncthreads();

    // ---- the verdict: uniform, before any store
    const uint32_t fd = s_first_data, ci = s_cont, nc = s_ncont;
    bool bad = s_bad != 0u || S.open_opcode > 2u || (mr.open_opcode != 0u && mr.open_len > FWS_MSG_MULTI_MAX_READ);
    // decode and join out of step
    bad = bad || nc > 1u || (nc == 1u && (S.open_opcode == 0u || ci != fd));
    bad = bad || (S.open_opcode != 0u && nc == 0u && (fd != kJnNone || mr.open_opcode != S.open_opcode));
    if (bad) {
        if (tid == 0) jn_result(a.res, rd, FWS_ERR_INVALID, 0u, 0u, 0u, 0u);
        return;
    }

    // ---- the state through the read's two appends (every thread the same scalars)
    const uint64_t H = a.stride >> 1;
    const uint64_t slot = (uint64_t)d.conn * a.stride;
    const uintptr_t dsp = (uintptr_t)a.dst + d.dst_off;
    uint32_t oo = S.open_opcode, hf = S.half & 1u, dr = S.dropped != 0u ? 1u : 0u;
    uint64_t ob = S.open_bytes, fl = dr ? 0u : S.fill, copied = 0u;
    JnJob job[2] = {{0u, 0u, 0u}, {0u, 0u, 0u}};
    // the CONTINUED entry's record
    uint64_t c_off = 0u, c_len = 0u;
    uint32_t c_where = FWS_JOIN_NOWHERE, c_flags = 0u;
    if (nc) {
        const uint32_t p = s_cont_len;
        ob += p;
        if (!dr) {
            if (fl > H || p > H - fl) dr = 1u, fl = 0u;
            else {
                if (p) job[0] = JnJob{dsp, (uintptr_t)a.store + slot + hf * H + fl, p};
                fl += p, copied += p;
            }
        }
        if (dr) c_where = FWS_JOIN_NOWHERE, c_off = 0u, c_len = ob, c_flags = FWS_JOIN_DROPPED;
        else c_where = FWS_JOIN_IN_STORE, c_off = slot + hf * H, c_len = fl, hf ^= 1u;
        oo = 0u, dr = 0u, ob = 0u, fl = 0u;
    }
    if (mr.open_opcode != 0u) {
        if (oo == 0u) oo = mr.open_opcode, dr = 0u, ob = 0u, fl = 0u;
        const uint32_t p = (uint32_t)mr.open_len;
        ob += p;
        if (!dr) {
            if (fl > H || p > H - fl) dr = 1u, fl = 0u;
            else {
                if (p) job[1] = JnJob{dsp + mr.open_off, (uintptr_t)a.store + slot + hf * H + fl, p};
                fl += p, copied += p;
            }
        }
    }

    // ---- the copies
    if (job[0].len) jn_copy<kThreads>(job[0], tid);
    if (job[1].len) jn_copy<kThreads>(job[1], tid);

    // ---- the records
#pragma unroll
    for (uint32_t k = 0; k < kIpt; ++k) {
        const uint32_t i = tid * kIpt + k;
        if (i >= mr.n_msgs) continue;
        fws_join_info x{};
        x.opcode = e[k].opcode;
        x.utf8_ok = e[k].utf8_ok;
        if (e[k].opcode >= 8u) {
            x.where = FWS_JOIN_IN_CTL, x.off = d.ctl_off + e[k].off, x.len = e[k].len;
            x.utf8_ok = 0;
        } else if (i == ci) {
            x.where = (uint8_t)c_where, x.off = c_off, x.len = c_len, x.flags = (uint8_t)c_flags;
        } else {
            x.where = FWS_JOIN_IN_DST, x.off = d.dst_off + e[k].off, x.len = e[k].len;
        }
        gput(a.joined + d.msg_base + i, x);
    }

    // ---- the result and the state, last
    if (tid == 0) {
        jn_result(a.res, rd, 0, mr.n_msgs, copied, oo, dr);
        fws_join_state n{};
        n.open_opcode = oo;
        n.half = hf;
        n.dropped = dr;
        n.open_bytes = ob;
        n.fill = fl;
        gput(state, n);
    }
}

}  // namespace fwsk

using namespace fwsk;

// Two forms by the decode call's max_len, as k_reply: up to 16 KiB 256 threads,
// above 1024.
constexpr uint32_t kJnSmallMax = 16u << 10;

int fws_launch_join(const fws_msg_read *reads, uint32_t n, uint32_t max_len, const fws_msg_info *msgs,
                    const uint8_t *dst, const fws_msg_result *mres, uint8_t *store, uint64_t store_stride,
                    fws_join_info *joined, fws_join_result *res, fws_join_state *states, uint32_t n_conns,
                    hipStream_t s) {
    static_assert(sizeof(fws_join_state) == 32 && sizeof(fws_join_info) == 32 && sizeof(fws_join_result) == 32,
                  "the ABI");
    if (!n) return 0;
    JnArgs a{store, dst, reads, msgs, mres, joined, res, states, store_stride, n_conns};
    if (max_len <= kJnSmallMax)
        hipLaunchKernelGGL((k_join<256u>), dim3(n), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((k_join<1024u>), dim3(n), dim3(1024), 0, s, a);
    return fws_hip_status(hipGetLastError());
}
