// msg_flow_kernels.hip -- fws_gpu_decode_messages_flow: the flow form of
// k_msg_multi (msg_multi_kernels.hip). The reads of many connections in one
// launch, one workgroup per read, with a per-connection state that also holds a
// data frame in progress: a read may begin inside a frame's payload and may end
// inside one, so a frame need not fit in a read and no read is declined for its
// header count.
//
// The four phases are k_msg_multi's -- stage the read in LDS, wave 0 walks the
// header chain and runs the message state machine, the workgroup gathers,
// unmasks and UTF-8-checks out of LDS, the entries / results / state go out --
// and nothing reaches global memory before the walk has ended; all but the walk
// are msg_small_common.h's (k_msg_multi calls its gather phase and spells the
// rest out, see there). What the flow form adds:
//   * the gather's elements are "the lead, then the frames taken": element 0 is
//     the payload of the frame in progress that opens the read (source offset 0,
//     the state's key, which is already rotated to its first byte; length 0 when
//     there is none), frame i is element i + 1. A data frame whose payload runs
//     past the read is an element of the bytes present. The per-frame tables
//     have one slot more for it; the frame records and the entries keep frame
//     indices.
//   * the walk starts at the lead's end and stops at header kMfFrames + 1 as at
//     an exceeded frame_cap, so the caller continues from resume_off.
//   * the state machine carries frame_unread / frame_len / frame_key /
//     frame_fin; a lead that ends a FIN frame completes the open message there.
// The UTF-8 regions live in dst byte space, so a cut inside a frame is nothing
// new to them: the lead belongs to the call's first (seeded) region.
//
// The stage's padding covers the windows the lead adds: the lead's windows start
// at source offset >= 0, a frame that begins inside a dst chunk reaches at most
// 15 bytes back (the zero chunk in front when its payload starts below 15), and
// the last window of an element that ends at N starts at or below N - 1 and ends
// below N + 20 <= 16 * nch + 32.
//
// kServer false is the client role (fws_gpu_decode_messages_flow_client): the
// header parse takes its client branch -- a MASK bit is FWS_ERR_MASKED, the
// header is 2, 4 or 10 bytes, the key is 0 -- and nothing else differs. The
// gather XORs with the zero key, so both roles run one copy of every phase and
// frame_key stays 0. The padding argument above holds with room to spare: a
// payload now starts at 2 or more, not 6, so a window still reaches at most 15
// bytes back (into the zero chunk), and a header window at the last offset
// reads the same 16 bytes behind it. What two-byte headers change is the count:
// a read of N bytes holds up to N / 2 headers, which the walk's stop at header
// kMfFrames + 1 bounds as before.
#include "fws_device.h"
#include "fws_internal.h"
#include "msg_small_common.h"

namespace fwsk {

constexpr uint32_t kMfNone = kMsNone;
constexpr uint32_t kMfFrames = kMsFrames;
constexpr uint32_t kMfElems = kMfFrames + 1u;   // the lead and the frames

struct MfArgs {
    const uint8_t *wire;
    const fws_msg_read *reads;
    fws_frame_info *frames;
    fws_msg_info *msgs;
    uint8_t *dst;
    uint8_t *ctl;
    fws_decode_result *res;
    fws_msg_result *mres;
    fws_msg_flow *flows;
    uint32_t n_conns;
    uint32_t max_len;
};

// what wave 0 leaves for the workgroup
struct MfHead {
    fws_decode_result res;
    fws_msg_result mres;
    fws_msg_flow next;           // but for msg.utf8_tail / msg.utf8_bad
    uint32_t nf;                 // frame records to write (<= frame_cap)
    uint32_t nel;                // elements: the lead and the frames the state machine took in
    uint32_t ne;                 // entries to write (<= msg_cap)
    uint32_t nreg;               // TEXT regions
    uint32_t over;               // a byte / entry capacity exceeded: no byte written, the state stays
    uint32_t db, cb;
    uint32_t open_cont;          // the carried message is still open
    uint32_t old_tail, old_bad;
};

template <uint32_t kStage, uint32_t kThreads, bool kServer>
__global__ __launch_bounds__(kThreads) void k_msg_flow(MfArgs a) {
    constexpr uint32_t kChunks = kStage / 16u;
    __shared__ u32x4 s_buf[kChunks + 3];            // a zero chunk in front, the read, two zero chunks
    __shared__ fws_frame_info s_fi[kMfFrames];
    __shared__ fws_msg_info s_ent[kMfFrames + 1];   // (a lead that completes a message, then one per frame)
    __shared__ uint32_t s_po[kMfElems];             // payload start of element f in the read
    __shared__ uint32_t s_key[kMfElems];
    __shared__ uint32_t s_dpre[kMfElems + 1];       // data bytes before element f (dst prefix)
    __shared__ uint32_t s_cpre[kMfElems + 1];       // control bytes before element f (ctl prefix)
    __shared__ uint32_t s_rlo[kMfFrames + 2];       // TEXT regions of dst, in dst order
    __shared__ uint32_t s_rhi[kMfFrames + 2];
    __shared__ uint32_t s_rmeta[kMfFrames + 2];
    __shared__ uint32_t s_rbad[kMfFrames + 2];
    __shared__ uint16_t s_ereg[kMfFrames + 2];      // entry -> its region, 0xFFFF: none
    __shared__ MfHead s_h;

    const uint32_t tid = threadIdx.x;
    const uint32_t rd = blockIdx.x;
    const fws_msg_read d = a.reads[rd];             // (a uniform address: scalar loads)
    if (const int32_t bad = ms_check_read(d, a.n_conns, a.max_len, kStage)) {
        if (tid == 0) ms_refuse(a.res, a.mres, rd, bad);
        return;
    }
    const uint32_t N = d.len;

    // 1. stage
    const uint8_t *sb = ms_stage<kChunks, kThreads>(s_buf, (uintptr_t)a.wire + d.wire_off, (N + 15u) >> 4, s_rbad,
                                                    kMfFrames + 2u, tid);

    // 2. the lead, the header chain and the message state machine (wave 0, uniformly)
    if (tid < kWave) {
        const uint32_t lane = tid;
        const fws_msg_flow old = a.flows[d.conn];
        fws_decode_result r{};
        r.status = FWS_OK;
        // the frame in progress: its first min(frame_unread, N) bytes open the read
        const uint64_t fu = old.frame_unread;
        const uint32_t lead = fu < N ? (uint32_t)fu : N;
        const bool inside = fu > N;                           // the read is all payload
        uint64_t pos = inside ? fu : lead;
        uint32_t nf = 0;
        bool capped = false;
        // the state before frame i (k_msg_plan's MsgScan, serially)
        uint32_t opc = old.msg.open_opcode & 0xFu;
        bool open = opc != 0, started = false, stop = false;
        uint32_t startf = kMfNone, fd = kMfNone, sb_ = lead, sf = 0, db = lead, cb = 0, nd = 0, ne = 0, np = 0, nreg = 0;
        uint32_t err_frame = kMfNone, end = lead;
        int32_t err_status = 0;
        uint64_t nfu = 0, nfl = 0;                            // the frame in progress at the end
        uint32_t nfk = 0, nff = 0;
        if (lane == 0) { s_po[0] = 0u; s_key[0] = old.frame_key; s_dpre[0] = 0u; s_cpre[0] = 0u; }
        if (inside) {
            nfu = fu - N; nfl = old.frame_len; nfk = rotr32(old.frame_key, 8u * (N & 3u)); nff = old.frame_fin;
        } else if (fu && old.frame_fin) {                     // the lead ends the message
            if (lane == 0) {
                fws_msg_info m{};
                m.off = 0; m.len = lead; m.first_frame = kMfNone; m.last_frame = kMfNone;
                m.n_data_frames = 0u; m.opcode = (uint8_t)opc; m.flags = (uint8_t)FWS_MSG_CONTINUED;
                s_ent[0] = m;
                s_ereg[0] = opc == 1u ? (uint16_t)0 : (uint16_t)0xFFFFu;
                if (opc == 1u) { s_rlo[0] = 0u; s_rhi[0] = lead; s_rmeta[0] = 0u | kMsSeeded; }
            }
            if (opc == 1u) ++nreg;
            ++ne;
            open = false;
        }
        while (pos < N) {
            Hdr h;
            const uint32_t q = (uint32_t)pos;
            const uint32_t bl = sb[q + (lane & 15u)];        // (in bounds: s_buf has a chunk past N)
            const int rc = parse_hdr([&](int i) -> uint32_t { return (uint32_t)__builtin_amdgcn_readlane((int)bl, i); },
                                     N - q, kServer, h);
            if (rc < 0) { r.status = rc; r.err_off = q; break; }
            if (rc == 0) break;                               // incomplete trailing header
            if (nf == kMfFrames) { capped = true; ++nf; break; }   // header kMfFrames + 1: the caller continues here
            const uint32_t i = nf;
            const uint32_t po = q + (uint32_t)rc;             // <= N
            const uint64_t pe = (uint64_t)po + h.plen;
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
                const uint32_t plen = trunc ? N - po : (uint32_t)h.plen;   // the bytes present
                if (h.opcode >= 8u) {
                    if (!h.fin || h.plen > 125u) {
                        err_frame = i; err_status = FWS_ERR_CONTROL_FRAME; end = q; stop = true;
                    } else if (trunc) {                       // control frames wait whole
                        end = q; stop = true;
                    } else {
                        if (lane == 0) {
                            fws_msg_info m{};
                            m.off = cb; m.len = plen; m.first_frame = i; m.last_frame = i; m.n_data_frames = 1u;
                            m.opcode = (uint8_t)h.opcode;
                            s_ent[ne] = m;
                            s_ereg[ne] = 0xFFFFu;
                            s_po[i + 1u] = po; s_key[i + 1u] = h.key; s_dpre[i + 1u] = db; s_cpre[i + 1u] = cb;
                        }
                        cb += plen; ++ne; ++np; end = (uint32_t)pe;
                    }
                } else if ((h.opcode == 0u) != open) {
                    err_frame = i; err_status = FWS_ERR_SEQUENCE; end = q; stop = true;
                } else {
                    if (h.opcode) { open = true; opc = h.opcode; started = true; startf = i; sb_ = 0; sf = 0; }
                    if (fd == kMfNone) fd = i;
                    if (lane == 0) { s_po[i + 1u] = po; s_key[i + 1u] = h.key; s_dpre[i + 1u] = db; s_cpre[i + 1u] = cb; }
                    db += plen; sb_ += plen; ++sf; ++nd; ++np;
                    if (trunc) {                              // taken as far as it is here; the rest is the next lead
                        end = N;
                        nfu = pe - N; nfl = h.plen; nfk = rotr32(h.key, 8u * (plen & 3u)); nff = h.fin;
                    } else {
                        end = (uint32_t)pe;
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
            }
            ++nf;
            pos = pe;
        }
        if (lane == 0) {
            MfHead hd{};
            if (r.status == FWS_OK) {
                if (capped) r.consumed = pos;                 // that header's offset
                else if (pos > N) { r.carry_unread = pos - N; r.consumed = N; }
                else if (pos < N) { r.carry_hdr_len = (uint32_t)(N - pos); r.consumed = pos; }
                else r.consumed = N;
            } else {
                r.consumed = r.err_off;
            }
            if ((nf > d.frame_cap || capped) && r.status == FWS_OK) r.status = FWS_ERR_CAPACITY;
            r.n_frames = nf;
            r.n_survivors = nf;
            const bool cont = open && !started;               // the carried message is still open
            const bool over = ne > d.msg_cap || db > d.dst_cap || cb > d.ctl_cap;
            fws_msg_result m{};
            m.n_msgs = ne;
            m.err_frame = err_frame;
            m.open_first_frame = open ? (cont ? fd : startf) : kMfNone;
            m.open_opcode = open ? opc : 0u;
            m.n_data_frames = nd;
            m.data_bytes = db;
            m.ctl_bytes = cb;
            m.open_off = open ? db - sb_ : 0u;
            m.open_len = open ? sb_ : 0u;
            m.resume_off = over ? 0u : end;
            m.status = err_status ? err_status : (r.status != 0 ? r.status : (over ? FWS_ERR_CAPACITY : 0));
            fws_msg_flow c{};
            c.msg.open_opcode = m.open_opcode;
            c.msg.open_frames = open ? (cont ? old.msg.open_frames : 0u) + sf : 0u;
            c.msg.open_bytes = open ? (cont ? old.msg.open_bytes : 0u) + sb_ : 0u;
            c.msg.prev_open_opcode = old.msg.open_opcode;
            c.msg.prev_open_frames = old.msg.open_frames;
            c.msg.prev_open_bytes = old.msg.open_bytes;
            c.msg.wire_bytes = old.msg.wire_bytes + end;
            c.msg.n_msgs = old.msg.n_msgs + ne;
            c.frame_unread = nfu;
            c.frame_len = nfl;
            c.frame_key = nfk;
            c.frame_fin = (uint8_t)nff;
            if (open && opc == 1u) {                           // the open TEXT part: the last region
                s_rlo[nreg] = db - sb_; s_rhi[nreg] = db;
                s_rmeta[nreg] = kMsEntry | kMsPrefix | (cont ? kMsSeeded : 0u);
                ++nreg;
            }
            s_dpre[np + 1u] = db;
            s_cpre[np + 1u] = cb;
            const uint32_t fcap = d.frame_cap < kMfFrames ? d.frame_cap : kMfFrames;
            hd.res = r;
            hd.mres = m;
            hd.next = c;
            hd.nf = nf < fcap ? nf : fcap;
            hd.nel = np + 1u;
            hd.ne = ne < d.msg_cap ? ne : d.msg_cap;
            hd.nreg = nreg;
            hd.over = over ? 1u : 0u;
            hd.db = db;
            hd.cb = cb;
            hd.open_cont = cont ? 1u : 0u;
            hd.old_tail = old.msg.utf8_tail;
            hd.old_bad = old.msg.utf8_bad;
            s_h = hd;
        }
    }
    __syncthreads();
    const uint32_t nreg = s_h.nreg;
    const bool over = s_h.over != 0;
    const MsTables t{sb, s_po, s_key, s_dpre, s_cpre, s_rlo, s_rhi, s_rmeta, s_rbad, s_h.nel};

    // the frame records (the walk's, whatever the message layer made of them)
    for (uint32_t i = tid; i < s_h.nf; i += kThreads) gput(a.frames + d.frame_base + i, s_fi[i]);

    // 3. gather + unmask, 4. UTF-8, the control payloads
    if (!over) ms_bulk<kThreads>(t, s_h.db, nreg, s_h.old_tail, a.dst + d.dst_off, a.ctl + d.ctl_off, tid);
    __syncthreads();

    // the entries with their verdicts, the results, the state
    ms_put_entries<kThreads>(t, s_ent, s_ereg, s_h.ne, over, s_h.old_bad, a.msgs + d.msg_base, tid);
    if (tid == 0) {
        if (!over) {
            fws_msg_flow c = s_h.next;
            if (c.msg.open_opcode == 1u) {
                const MsOpenText o = ms_open_text(t, nreg, s_h.open_cont != 0u, s_h.old_tail, s_h.old_bad);
                c.msg.utf8_bad = o.bad;
                c.msg.utf8_tail = o.tail;
            }
            gput(a.flows + d.conn, c);
        }
        gput(a.res + rd, s_h.res);
        gput(a.mres + rd, s_h.mres);
    }
}

}  // namespace fwsk

using namespace fwsk;

// The two forms of k_msg_multi: a 16 KiB stage at 256 threads, several workgroups
// to a CU; kSmallMax at 1024 threads, one workgroup to a CU.
constexpr uint32_t kMfSmallStage = 16u << 10;

int fws_launch_msg_flow(const uint8_t *wire, const fws_msg_read *reads, uint32_t n, uint32_t max_len,
                        fws_frame_info *frames, fws_msg_info *msgs, uint8_t *dst, uint8_t *ctl,
                        fws_decode_result *res, fws_msg_result *mres, fws_msg_flow *flows, uint32_t n_conns,
                        hipStream_t s, bool client) {
    static_assert(FWS_MSG_MULTI_MAX_READ == kSmallMax && FWS_MSG_MULTI_MAX_FRAMES == kSmallFrames, "the small-read limits");
    static_assert(sizeof(fws_msg_flow) == 96 && offsetof(fws_msg_flow, frame_unread) == 64, "the state's layout");
    if (!n) return 0;
    MfArgs a{wire, reads, frames, msgs, dst, ctl, res, mres, flows, n_conns, max_len};
    if (client) {
        if (max_len <= kMfSmallStage)
            hipLaunchKernelGGL((k_msg_flow<kMfSmallStage, 256u, false>), dim3(n), dim3(256), 0, s, a);
        else
            hipLaunchKernelGGL((k_msg_flow<(uint32_t)kSmallMax, 1024u, false>), dim3(n), dim3(1024), 0, s, a);
    } else if (max_len <= kMfSmallStage)
        hipLaunchKernelGGL((k_msg_flow<kMfSmallStage, 256u, true>), dim3(n), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((k_msg_flow<(uint32_t)kSmallMax, 1024u, true>), dim3(n), dim3(1024), 0, s, a);
    return fws_hip_status(hipGetLastError());
}
