// msg_multi_kernels.hip -- fws_gpu_decode_messages_multi: the reads of many
// connections decoded into messages in one launch, one workgroup per read.
//
// fws_gpu_decode_messages_carry is nine launches per connection (k_scan ...
// k_utf8_msgs), built for HBM-sized streams; a server's loop step brings reads
// of a few KiB from hundreds of connections. Here each read is staged in LDS
// as decode_small_wg stages it (small_kernels.hip), wave 0 walks its header
// chain from offset 0 with parse_hdr by readlane and runs the message state
// machine of k_msg_plan in the same loop -- at most kSmallFrames frames, so the
// grouping needs no scan: the state before frame i is in registers --, and the
// whole workgroup then gathers, unmasks and UTF-8-checks out of LDS. Per read
// the outputs are those of fws_gpu_decode_messages_carry on that read alone
// (n_survivors = n_frames, as decode_small_wg reports it).
//
// Nothing is written to global memory before the walk has ended: the frame
// records and the entries are built in LDS, so a read declined for its header
// count leaves only its two results, and the byte / entry overflow verdict is
// known before the first payload byte is stored.
//
// The gather / unmask / UTF-8 phase and the control payloads are
// msg_small_common.h's ms_bulk, shared with k_msg_flow; here an element is a
// frame. The descriptor checks, the staging and the write-out are spelled out
// below although the header has them (ms_check_read, ms_stage, ms_put_entries,
// ms_open_text: k_msg_flow's): with any of the three called from the header the
// 1024-thread form measured 0.2 to 2.3 us slower at 64 KiB reads, the serial
// walk's code moving with the register allocation around it (DESIGN.md 4.7.3,
// "One copy of the shared phases"). A fix to one of them goes into both places.
// The UTF-8 regions are the completed TEXT entries and the open TEXT part, as in
// k_utf8_msgs<true>: the carried tail is the left context of a region that
// began in an earlier call, the open part counts only errors at its own byte
// positions.
#include "fws_device.h"
#include "fws_internal.h"
#include "msg_small_common.h"

namespace fwsk {

constexpr uint32_t kMmNone = kMsNone;
constexpr uint32_t kMmFrames = kMsFrames;

struct MmArgs {
    const uint8_t *wire;
    const fws_msg_read *reads;
    fws_frame_info *frames;
    fws_msg_info *msgs;
    uint8_t *dst;
    uint8_t *ctl;
    fws_decode_result *res;
    fws_msg_result *mres;
    fws_msg_carry *carries;
    uint32_t n_conns;
    uint32_t max_len;
};

// what wave 0 leaves for the workgroup
struct MmHead {
    fws_decode_result res;
    fws_msg_result mres;
    fws_msg_carry next;          // but for utf8_tail / utf8_bad
    uint32_t mode;               // 0: decoded; else both results carry this status and nothing else is written
    uint32_t nf;                 // frame records to write (<= frame_cap)
    uint32_t np;                 // frames the state machine took in
    uint32_t ne;                 // entries to write (<= msg_cap)
    uint32_t nreg;               // TEXT regions
    uint32_t over;               // a byte / entry capacity exceeded: no byte written, the carry stays
    uint32_t db, cb;
    uint32_t open_cont;          // the carried message is still open
    uint32_t old_tail, old_bad;
};

template <uint32_t kStage, uint32_t kThreads>
__global__ __launch_bounds__(kThreads) void k_msg_multi(MmArgs a) {
    constexpr uint32_t kChunks = kStage / 16u;
    __shared__ u32x4 s_buf[kChunks + 3];            // a zero chunk in front, the read, two zero chunks
    __shared__ fws_frame_info s_fi[kMmFrames];
    __shared__ fws_msg_info s_ent[kMmFrames];
    __shared__ uint32_t s_po[kMmFrames];            // payload start of frame f in the read
    __shared__ uint32_t s_key[kMmFrames];
    __shared__ uint32_t s_dpre[kMmFrames + 1];      // data bytes before frame f (dst prefix)
    __shared__ uint32_t s_cpre[kMmFrames + 1];      // control bytes before frame f (ctl prefix)
    __shared__ uint32_t s_rlo[kMmFrames + 1];       // TEXT regions of dst, in dst order
    __shared__ uint32_t s_rhi[kMmFrames + 1];
    __shared__ uint32_t s_rmeta[kMmFrames + 1];
    __shared__ uint32_t s_rbad[kMmFrames + 1];
    __shared__ uint16_t s_ereg[kMmFrames];          // entry -> its region, 0xFFFF: none
    __shared__ MmHead s_h;

    const uint32_t tid = threadIdx.x;
    const uint32_t rd = blockIdx.x;
    const fws_msg_read d = a.reads[rd];             // (a uniform address: scalar loads)
    // (ms_check_read's text)
    if ((d.wire_off & 15u) || (d.dst_off & 15u) || d.conn >= a.n_conns) {
        if (tid == 0) ms_refuse(a.res, a.mres, rd, FWS_ERR_INVALID);
        return;
    }
    if (d.len > a.max_len || d.len > FWS_MSG_MULTI_MAX_READ || d.len > kStage) {
        if (tid == 0) ms_refuse(a.res, a.mres, rd, FWS_ERR_DECLINED);
        return;
    }
    const uint32_t N = d.len;
    const uint32_t nch = (N + 15u) >> 4;
    const uintptr_t base = (uintptr_t)a.wire + d.wire_off;

    // 1. stage (ms_stage's text): all loads of a thread in flight together
    static_assert(kChunks % (4u * kThreads) == 0, "staging rounds of four loads per thread");
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
    for (uint32_t i = tid; i <= kMsFrames; i += kThreads) s_rbad[i] = 0u;
    __syncthreads();
    // byte 0 of the read; a header window at the last offset and a 20-byte payload
    // window that starts up to 15 bytes before a payload or ends at N stay in s_buf
    const uint8_t *sb = (const uint8_t *)(s_buf + 1);
    static_assert(sizeof(s_buf) >= kStage + 48u, "one chunk in front of the read, two behind");

    // 2. the header chain and the message state machine (wave 0, uniformly)
    if (tid < kWave) {
        const uint32_t lane = tid;
        const fws_msg_carry old = a.carries[d.conn];
        fws_decode_result r{};
        r.status = FWS_OK;
        uint64_t pos = 0;
        uint32_t nf = 0;
        bool declined = false;
        // the state before frame i (k_msg_plan's MsgScan, serially)
        uint32_t opc = old.open_opcode & 0xFu;
        bool open = opc != 0, started = false, stop = false;
        uint32_t startf = kMmNone, fd = kMmNone, sb_ = 0, sf = 0, db = 0, cb = 0, nd = 0, ne = 0, np = 0, nreg = 0;
        uint32_t err_frame = kMmNone, end = 0;
        int32_t err_status = 0;
        while (pos < N) {
            Hdr h;
            const uint32_t q = (uint32_t)pos;
            const uint32_t bl = sb[q + (lane & 15u)];        // (in bounds: s_buf has a chunk past N)
            const int rc = parse_hdr([&](int i) -> uint32_t { return (uint32_t)__builtin_amdgcn_readlane((int)bl, i); },
                                     N - q, true, h);
            if (rc < 0) { r.status = rc; r.err_off = q; break; }
            if (rc == 0) break;                               // incomplete trailing header
            if (nf == kMmFrames) { declined = true; break; }
            const uint32_t i = nf;
            const uint64_t po = q + (uint32_t)rc;
            const uint64_t pe = po + h.plen;
            const bool trunc = pe > N;
            if (lane == 0) {
                fws_frame_info fi;
                fi.hdr_off = q; fi.payload_len = h.plen; fi.key = h.key; fi.opcode = (uint8_t)h.opcode;
                fi.fin = (uint8_t)h.fin; fi.hdr_len = (uint8_t)rc;
                fi.flags = trunc ? (uint8_t)FWS_FRAME_TRUNCATED : (uint8_t)0;
                s_fi[i] = fi;
            }
            if (!stop && i >= d.frame_cap) stop = true;       // the first frame_cap frames are grouped
            if (!stop) {
                const uint32_t plen = (uint32_t)h.plen;       // (used when the frame is whole: <= N)
                if (h.opcode >= 8u) {
                    if (!h.fin || h.plen > 125u) {
                        err_frame = i; err_status = FWS_ERR_CONTROL_FRAME; end = q; stop = true;
                    } else if (trunc) {                       // whole frames only
                        end = q; stop = true;
                    } else {
                        if (lane == 0) {
                            fws_msg_info m{};
                            m.off = cb; m.len = plen; m.first_frame = i; m.last_frame = i; m.n_data_frames = 1u;
                            m.opcode = (uint8_t)h.opcode;
                            s_ent[ne] = m;
                            s_ereg[ne] = 0xFFFFu;
                            s_po[i] = (uint32_t)po; s_key[i] = h.key; s_dpre[i] = db; s_cpre[i] = cb;
                        }
                        cb += plen; ++ne; ++np; end = (uint32_t)pe;
                    }
                } else if (trunc) {
                    end = q; stop = true;
                } else if ((h.opcode == 0u) != open) {
                    err_frame = i; err_status = FWS_ERR_SEQUENCE; end = q; stop = true;
                } else {
                    if (h.opcode) { open = true; opc = h.opcode; started = true; startf = i; sb_ = 0; sf = 0; }
                    if (fd == kMmNone) fd = i;
                    if (lane == 0) { s_po[i] = (uint32_t)po; s_key[i] = h.key; s_dpre[i] = db; s_cpre[i] = cb; }
                    db += plen; sb_ += plen; ++sf; ++nd; ++np; end = (uint32_t)pe;
                    if (h.fin) {
                        if (lane == 0) {
                            fws_msg_info m{};
                            m.off = db - sb_; m.len = sb_; m.first_frame = started ? startf : fd; m.last_frame = i;
                            m.n_data_frames = sf; m.opcode = (uint8_t)opc;
                            m.flags = started ? (uint8_t)0 : (uint8_t)FWS_MSG_CONTINUED;
                            s_ent[ne] = m;
                            s_ereg[ne] = opc == 1u ? (uint16_t)nreg : (uint16_t)0xFFFFu;
                            if (opc == 1u) {
                                s_rlo[nreg] = db - sb_; s_rhi[nreg] = db;
                                s_rmeta[nreg] = ne | (started ? 0u : kMsSeeded);
                            }
                        }
                        if (opc == 1u) ++nreg;
                        ++ne;
                        open = false;
                    }
                }
            }
            ++nf;
            pos = pe;
        }
        if (lane == 0) {
            MmHead hd{};
            if (declined) {
                hd.mode = (uint32_t)FWS_ERR_DECLINED;
            } else {
                if (r.status == FWS_OK) {
                    if (pos > N) { r.carry_unread = pos - N; r.consumed = N; }
                    else if (pos < N) { r.carry_hdr_len = (uint32_t)(N - pos); r.consumed = pos; }
                    else r.consumed = N;
                } else {
                    r.consumed = r.err_off;
                }
                if (nf > d.frame_cap && r.status == FWS_OK) r.status = FWS_ERR_CAPACITY;
                r.n_frames = nf;
                r.n_survivors = nf;
                const bool cont = open && !started;           // the carried message is still open
                const bool over = ne > d.msg_cap || db > d.dst_cap || cb > d.ctl_cap;
                fws_msg_result m{};
                m.n_msgs = ne;
                m.err_frame = err_frame;
                m.open_first_frame = open ? (cont ? fd : startf) : kMmNone;
                m.open_opcode = open ? opc : 0u;
                m.n_data_frames = nd;
                m.data_bytes = db;
                m.ctl_bytes = cb;
                m.open_off = open ? db - sb_ : 0u;
                m.open_len = open ? sb_ : 0u;
                m.resume_off = over ? 0u : end;
                m.status = err_status ? err_status : (r.status != 0 ? r.status : (over ? FWS_ERR_CAPACITY : 0));
                fws_msg_carry c{};
                c.open_opcode = m.open_opcode;
                c.open_frames = open ? (cont ? old.open_frames : 0u) + sf : 0u;
                c.open_bytes = open ? (cont ? old.open_bytes : 0u) + sb_ : 0u;
                c.prev_open_opcode = old.open_opcode;
                c.prev_open_frames = old.open_frames;
                c.prev_open_bytes = old.open_bytes;
                c.wire_bytes = old.wire_bytes + end;
                c.n_msgs = old.n_msgs + ne;
                if (open && opc == 1u) {                       // the open TEXT part: the last region
                    s_rlo[nreg] = db - sb_; s_rhi[nreg] = db;
                    s_rmeta[nreg] = kMsEntry | kMsPrefix | (cont ? kMsSeeded : 0u);
                    ++nreg;
                }
                s_dpre[np] = db;
                s_cpre[np] = cb;
                hd.res = r;
                hd.mres = m;
                hd.next = c;
                hd.nf = nf < d.frame_cap ? nf : d.frame_cap;
                hd.np = np;
                hd.ne = ne < d.msg_cap ? ne : d.msg_cap;
                hd.nreg = nreg;
                hd.over = over ? 1u : 0u;
                hd.db = db;
                hd.cb = cb;
                hd.open_cont = cont ? 1u : 0u;
                hd.old_tail = old.utf8_tail;
                hd.old_bad = old.utf8_bad;
            }
            s_h = hd;
        }
    }
    __syncthreads();
    if (s_h.mode) {
        if (tid == 0) ms_refuse(a.res, a.mres, rd, (int32_t)s_h.mode);
        return;
    }
    const uint32_t nreg = s_h.nreg;
    const bool over = s_h.over != 0;
    const MsTables t{sb, s_po, s_key, s_dpre, s_cpre, s_rlo, s_rhi, s_rmeta, s_rbad, s_h.np};

    // the frame records (the walk's, whatever the message layer made of them)
    for (uint32_t i = tid; i < s_h.nf; i += kThreads) gput(a.frames + d.frame_base + i, s_fi[i]);

    // 3. gather + unmask, 4. UTF-8, the control payloads
    if (!over) ms_bulk<kThreads>(t, s_h.db, nreg, s_h.old_tail, a.dst + d.dst_off, a.ctl + d.ctl_off, tid);
    __syncthreads();

    // the entries with their verdicts (ms_put_entries' text), the results, the carry (ms_open_text's text)
    for (uint32_t e = tid; e < s_h.ne; e += kThreads) {
        fws_msg_info m = s_ent[e];
        const uint32_t g = s_ereg[e];
        if (!over && g != 0xFFFFu)
            m.utf8_ok = (s_rbad[g] || ((s_rmeta[g] & kMsSeeded) && s_h.old_bad)) ? (uint8_t)0 : (uint8_t)1;
        gput(a.msgs + d.msg_base + e, m);
    }
    if (tid == 0) {
        if (!over) {
            fws_msg_carry c = s_h.next;
            if (c.open_opcode == 1u) {
                const uint32_t g = nreg - 1u, rl = s_rlo[g], rh = s_rhi[g];
                c.utf8_bad = (s_rbad[g] || (s_h.open_cont && s_h.old_bad)) ? 1u : 0u;
                uint32_t tl = s_h.open_cont ? s_h.old_tail : 0u;
                uint32_t k = rh - rl > 3u ? rh - 3u : rl;
                if (k < rh) {
                    uint32_t f = ms_owner(t, k);
                    for (; k < rh; ++k) tl = (tl >> 8) | (ms_dst_byte(t, k, f) << 24);
                }
                c.utf8_tail = tl & 0xFFFFFF00u;
            }
            gput(a.carries + d.conn, c);
        }
        gput(a.res + rd, s_h.res);
        gput(a.mres + rd, s_h.mres);
    }
}

}  // namespace fwsk

using namespace fwsk;

// The small form: a 16 KiB stage at 256 threads, several workgroups to a CU;
// the full form: kSmallMax at 1024 threads, one workgroup to a CU.
constexpr uint32_t kMmSmallStage = 16u << 10;

int fws_launch_msg_multi(const uint8_t *wire, const fws_msg_read *reads, uint32_t n, uint32_t max_len,
                         fws_frame_info *frames, fws_msg_info *msgs, uint8_t *dst, uint8_t *ctl,
                         fws_decode_result *res, fws_msg_result *mres, fws_msg_carry *carries, uint32_t n_conns,
                         hipStream_t s) {
    static_assert(FWS_MSG_MULTI_MAX_READ == kSmallMax && FWS_MSG_MULTI_MAX_FRAMES == kSmallFrames, "the small-read limits");
    if (!n) return 0;
    MmArgs a{wire, reads, frames, msgs, dst, ctl, res, mres, carries, n_conns, max_len};
    if (max_len <= kMmSmallStage)
        hipLaunchKernelGGL((k_msg_multi<kMmSmallStage, 256u>), dim3(n), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((k_msg_multi<(uint32_t)kSmallMax, 1024u>), dim3(n), dim3(1024), 0, s, a);
    return fws_hip_status(hipGetLastError());
}
