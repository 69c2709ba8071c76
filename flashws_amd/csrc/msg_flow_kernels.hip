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
// and nothing reaches global memory before the walk has ended. What the flow
// form adds:
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
#include "fws_device.h"
#include "fws_internal.h"

namespace fwsk {

constexpr uint32_t kMfNone = 0xFFFFFFFFu;
constexpr uint32_t kMfFrames = kSmallFrames;
constexpr uint32_t kMfElems = kMfFrames + 1u;   // the lead and the frames
constexpr uint32_t kMfSeeded = 1u << 16;     // region meta: the carried tail is its left context
constexpr uint32_t kMfPrefix = 1u << 17;     // region meta: the open part (errors inside it only)
constexpr uint32_t kMfEntry = 0xFFFFu;       // region meta: its entry

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

__device__ __forceinline__ void mf_refuse(const MfArgs &a, uint32_t r, int32_t status) {
    fws_decode_result d{};
    d.status = status;
    fws_msg_result m{};
    m.status = status;
    m.err_frame = kMfNone;
    m.open_first_frame = kMfNone;
    gput(a.res + r, d);
    gput(a.mres + r, m);
}

template <uint32_t kStage, uint32_t kThreads>
__global__ __launch_bounds__(kThreads) void k_msg_flow(MfArgs a) {
    constexpr uint32_t kChunks = kStage / 16u;
    static_assert(kChunks % (4u * kThreads) == 0, "staging rounds of four loads per thread");
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
    if ((d.wire_off & 15u) || (d.dst_off & 15u) || d.conn >= a.n_conns) {
        if (tid == 0) mf_refuse(a, rd, FWS_ERR_INVALID);
        return;
    }
    const uint32_t N = d.len;
    if (N > a.max_len || N > FWS_MSG_MULTI_MAX_READ || N > kStage) {
        if (tid == 0) mf_refuse(a, rd, FWS_ERR_DECLINED);
        return;
    }
    const uint32_t nch = (N + 15u) >> 4;
    const uintptr_t base = (uintptr_t)a.wire + d.wire_off;

    // 1. stage: all loads of a thread in flight together (decode_small_wg step 1)
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
    for (uint32_t i = tid; i < kMfFrames + 2u; i += kThreads) s_rbad[i] = 0u;
    __syncthreads();
    // byte 0 of the read; a header window at the last offset and a 20-byte payload
    // window that starts up to 15 bytes before a payload or ends at N stay in s_buf:
    // the lead's windows start at source offset >= 0, a frame that begins inside a
    // dst chunk reaches at most 15 bytes back (the zero chunk in front when its
    // payload starts below 15), and the last window of an element that ends at N
    // starts at or below N - 1 and ends below N + 20 <= 16 * nch + 32
    const uint8_t *sb = (const uint8_t *)(s_buf + 1);
    static_assert(sizeof(s_buf) >= kStage + 48u, "one chunk in front of the read, two behind");

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
                if (opc == 1u) { s_rlo[0] = 0u; s_rhi[0] = lead; s_rmeta[0] = 0u | kMfSeeded; }
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
                                     N - q, true, h);
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
                                    s_rmeta[nreg] = ne | (started ? 0u : kMfSeeded);
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
                s_rmeta[nreg] = kMfEntry | kMfPrefix | (cont ? kMfSeeded : 0u);
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
    const uint32_t nel = s_h.nel, db = s_h.db, nreg = s_h.nreg;
    const bool over = s_h.over != 0;
    const uint32_t old_tail = s_h.old_tail;

    // the frame records (the walk's, whatever the message layer made of them)
    for (uint32_t i = tid; i < s_h.nf; i += kThreads) gput(a.frames + d.frame_base + i, s_fi[i]);

    // the unmasked byte at dst offset y < db; f: an element at or before its owner
    auto dst_byte = [&](uint32_t y, uint32_t &f) -> uint32_t {
        while (s_dpre[f + 1u] <= y) ++f;
        const uint32_t k = y - s_dpre[f];
        return (uint32_t)sb[s_po[f] + k] ^ ((s_key[f] >> (8u * (k & 3u))) & 0xFFu);
    };
    // the owner of dst byte x < db: the last element whose dst prefix is <= x
    auto owner = [&](uint32_t x) -> uint32_t {
        uint32_t lo = 0, hi = nel - 1u;
        while (lo < hi) {
            const uint32_t m = (lo + hi + 1u) >> 1;
            if (s_dpre[m] <= x) lo = m; else hi = m - 1u;
        }
        return lo;
    };

    // dst chunk [x0, x0 + 16), zeros from db on: per element that meets it, the 16-B
    // source window at the chunk's offset in that element -- five aligned dwords from
    // LDS shifted to the source phase; the window may start up to 15 bytes before
    // the payload or run past its end, into staged bytes the select drops --, the
    // key rotated to the chunk's payload phase, the element's bytes selected.
    auto dst_chunk = [&](uint32_t x0) -> u32x4 {
        u32x4 v{0u, 0u, 0u, 0u};
        if (x0 >= db) return v;
        for (uint32_t f = owner(x0); f < nel && s_dpre[f] < x0 + 16u; ++f) {
            const uint32_t b = s_dpre[f], e = s_dpre[f + 1u];
            if (e == b) continue;                            // a control frame, an empty fragment, no lead
            const uint32_t k = x0 - b;                       // (mod 2^32 when the element starts inside the chunk)
            const int32_t s = (int32_t)s_po[f] + (int32_t)k; // >= -15
            const uint32_t sh = (uint32_t)s & 3u;
            const uint32_t *w = (const uint32_t *)(sb + (s & ~3));
            const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
            const uint32_t rk = rotr32(s_key[f], 8u * (k & 3u));
            v.x |= (__builtin_amdgcn_alignbyte(w1, w0, sh) ^ rk) & sel_bytes(x0, b, e);
            v.y |= (__builtin_amdgcn_alignbyte(w2, w1, sh) ^ rk) & sel_bytes(x0 + 4u, b, e);
            v.z |= (__builtin_amdgcn_alignbyte(w3, w2, sh) ^ rk) & sel_bytes(x0 + 8u, b, e);
            v.w |= (__builtin_amdgcn_alignbyte(w4, w3, sh) ^ rk) & sel_bytes(x0 + 12u, b, e);
        }
        return v;
    };

    if (!over) {
        // 3. gather + unmask, 4. UTF-8 on the chunk in registers. Chunks run to
        //    db + 3 so an unfinished sequence at the end meets zero bytes. A wave
        //    takes 64 * steps consecutive chunks: the dword before a lane's chunk is
        //    its neighbour's last (lane 0: lane 63's of the step before; the wave's
        //    first chunk: assembled once more).
        uint8_t *const out = a.dst + d.dst_off;
        const uint32_t nck = (db + 18u) >> 4;
        const uint32_t steps = (nck + kThreads - 1u) / kThreads;
        const uint32_t wlane = tid & (kWave - 1u);
        uint32_t carry = 0;
        for (uint32_t st = 0; st < steps; ++st) {            // (the same trips for every lane: the shuffles below)
            const uint32_t c = ((tid / kWave) * steps + st) * kWave + wlane;
            const uint32_t x0 = 16u * c;
            const u32x4 v = c < nck ? dst_chunk(x0) : u32x4{0u, 0u, 0u, 0u};
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
                const u32x4 pv = c && c < nck ? dst_chunk(x0 - 16u) : u32x4{0u, 0u, 0u, 0u};
                if (wlane == 0) prev = pv.w;
            }
            if (c >= nck) continue;
            // ASCII through and through: no region can flag anything here
            if (!((v.x | v.y | v.z | v.w | (c ? prev : old_tail)) & 0x80808080u)) continue;
            // the first region with hi + 3 > x0; the regions that meet the chunk follow it
            uint32_t lo = 0, hi = nreg;
            while (lo < hi) {
                const uint32_t m = (lo + hi) >> 1;
                if (s_rhi[m] + 3u > x0) hi = m; else lo = m + 1u;
            }
            for (uint32_t g = lo; g < nreg && (s_rlo[g] >> 4) <= c; ++g) {
                const uint32_t rl = s_rlo[g], rh = s_rhi[g], meta = s_rmeta[g];
                const uint32_t sx = sel_bytes(x0, rl, rh), sy = sel_bytes(x0 + 4u, rl, rh);
                const uint32_t sz = sel_bytes(x0 + 8u, rl, rh), sw = sel_bytes(x0 + 12u, rl, rh);
                const uint32_t vx = v.x & sx, vy = v.y & sy, vz = v.z & sz, vw = v.w & sw;
                const uint32_t p = c ? prev & sel_bytes(x0 - 4u, rl, rh) : ((meta & kMfSeeded) ? old_tail : 0u);
                if (!((vx | vy | vz | vw | p) & 0x80808080u)) continue;
                uint32_t bad;
                if (meta & kMfPrefix)
                    bad = (utf8_err(vx, p) & sx) | (utf8_err(vy, vx) & sy) | (utf8_err(vz, vy) & sz) |
                          (utf8_err(vw, vz) & sw);
                else
                    bad = utf8_err(vx, p) | utf8_err(vy, vx) | utf8_err(vz, vy) | utf8_err(vw, vz);
                if (bad) s_rbad[g] = 1u;
            }
        }
        // the control payloads: a wave per control frame taken in
        uint8_t *const cout = a.ctl + d.ctl_off;
        const uint32_t lane = tid & (kWave - 1u);
        for (uint32_t f = tid / kWave; f < nel; f += kThreads / kWave) {
            const uint32_t co = s_cpre[f], cl = s_cpre[f + 1u] - co;
            for (uint32_t k = lane; k < cl; k += kWave)
                gput(cout + co + k, (uint8_t)(sb[s_po[f] + k] ^ (uint8_t)(s_key[f] >> (8u * (k & 3u)))));
        }
    }
    __syncthreads();

    // the entries with their verdicts, the results, the state
    for (uint32_t e = tid; e < s_h.ne; e += kThreads) {
        fws_msg_info m = s_ent[e];
        const uint32_t g = s_ereg[e];
        if (!over && g != 0xFFFFu)
            m.utf8_ok = (s_rbad[g] || ((s_rmeta[g] & kMfSeeded) && s_h.old_bad)) ? (uint8_t)0 : (uint8_t)1;
        gput(a.msgs + d.msg_base + e, m);
    }
    if (tid == 0) {
        if (!over) {
            fws_msg_flow c = s_h.next;
            if (c.msg.open_opcode == 1u) {
                const uint32_t g = nreg - 1u, rl = s_rlo[g], rh = s_rhi[g];
                c.msg.utf8_bad = (s_rbad[g] || (s_h.open_cont && s_h.old_bad)) ? 1u : 0u;
                uint32_t t = s_h.open_cont ? old_tail : 0u;
                uint32_t k = rh - rl > 3u ? rh - 3u : rl;
                if (k < rh) {
                    uint32_t f = owner(k);
                    for (; k < rh; ++k) t = (t >> 8) | (dst_byte(k, f) << 24);
                }
                c.msg.utf8_tail = t & 0xFFFFFF00u;
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
                        hipStream_t s) {
    static_assert(FWS_MSG_MULTI_MAX_READ == kSmallMax && FWS_MSG_MULTI_MAX_FRAMES == kSmallFrames, "the small-read limits");
    static_assert(sizeof(fws_msg_flow) == 96 && offsetof(fws_msg_flow, frame_unread) == 64, "the state's layout");
    if (!n) return 0;
    MfArgs a{wire, reads, frames, msgs, dst, ctl, res, mres, flows, n_conns, max_len};
    if (max_len <= kMfSmallStage)
        hipLaunchKernelGGL((k_msg_flow<kMfSmallStage, 256u>), dim3(n), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((k_msg_flow<(uint32_t)kSmallMax, 1024u>), dim3(n), dim3(1024), 0, s, a);
    return fws_hip_status(hipGetLastError());
}
