// fws_abi.hip -- the extern "C" entry points of libfws_gpu.so (include/fws_gpu.h).
// Host code: argument checks, workspace ownership, kernel launch sequencing.
#include <stdlib.h>
#include <string.h>

#include "fws_internal.h"

namespace {

template <typename T>
int dev_alloc(T **p, uint64_t count) {
    *p = nullptr;
    if (count == 0) count = 1;
    return fws_hip_status(hipMalloc((void **)p, count * sizeof(T)));
}

template <typename T>
void dev_free(T *&p) {
    if (p) (void)hipFree(p);
    p = nullptr;
}

void free_plan(fws_plan_ws &w) {
    dev_free(w.block_sums);
    dev_free(w.cbase);
    dev_free(w.unit_first);
    dev_free(w.unit_rec);
    dev_free(w.total);
    dev_free(w.status);
    dev_free(w.ticket);
    dev_free(w.mode);
    dev_free(w.tx_seam);
}

}  // namespace

int fws_ctx_ensure_plan(fws_gpu_ctx *ctx, uint64_t frames, uint64_t units) {
    if (frames <= ctx->cap_frames && units <= ctx->cap_units && ctx->plan.cbase) return 0;
    if (frames < ctx->cap_frames) frames = ctx->cap_frames;
    if (units < ctx->cap_units) units = ctx->cap_units;
    free_plan(ctx->plan);
    int r;
    if ((r = dev_alloc(&ctx->plan.block_sums, frames / 1024 + 2))) return r;
    if ((r = dev_alloc(&ctx->plan.cbase, frames + 2))) return r;
    if ((r = dev_alloc(&ctx->plan.unit_first, units + 2))) return r;
    if ((r = dev_alloc(&ctx->plan.unit_rec, 4 * (units + 2)))) return r;
    if ((r = dev_alloc(&ctx->plan.total, 2))) return r;
    if ((r = dev_alloc(&ctx->plan.status, frames / 8 + 2))) return r;
    if ((r = dev_alloc(&ctx->plan.ticket, 2))) return r;
    if ((r = dev_alloc(&ctx->plan.mode, sizeof(fws_plan_mode) / 8))) return r;
    if ((r = dev_alloc(&ctx->plan.tx_seam, 4 * (2 * frames + 2)))) return r;
    if ((r = fws_hip_status(hipMemset(ctx->plan.status, 0, (frames / 8 + 2) * 8)))) return r;
    if ((r = fws_hip_status(hipMemset(ctx->plan.ticket, 0, 8)))) return r;
    if ((r = fws_hip_status(hipMemset(ctx->plan.mode, 0, sizeof(fws_plan_mode))))) return r;
    ctx->plan.status_cap = frames / 8 + 2;             // k_tx_one: >= 8 frames per workgroup
    ctx->plan.epoch = 0;
    ctx->cap_frames = frames;
    ctx->cap_units = units;
    ctx->plan.unit_cap = units + 1;
    return 0;
}

// per-unit seam words of fws_gpu_unmask_sorted_utf8 for a span of `span` bytes
int fws_ctx_ensure_seam(fws_gpu_ctx *ctx, uint64_t span) {
    const uint64_t words = 2 * (span / 4096 + 2);
    if (words <= ctx->seam_cap) return 0;
    dev_free(ctx->seam);
    ctx->seam_cap = 0;
    if (int r = fws_hip_status(hipMalloc((void **)&ctx->seam, words * 4))) return r;
    ctx->seam_cap = words;
    return 0;
}

// the message planner's workspace for `frames` frames (fws_gpu_decode_messages)
int fws_ctx_ensure_msg(fws_gpu_ctx *ctx, uint64_t frames) {
    fws_msg_ws &m = ctx->msg;
    if (!m.cnext) {
        if (int r = dev_alloc(&m.cnext, 1)) return r;
    }
    if (frames <= m.cap && m.descs) return 0;
    if (frames < m.cap) frames = m.cap;
    dev_free(m.descs);
    dev_free(m.ctl_off);
    dev_free(m.agg);
    dev_free(m.pre);
    m.cap = 0;
    int r;
    if ((r = dev_alloc(&m.descs, frames + 1))) return r;
    if ((r = dev_alloc(&m.ctl_off, frames + 1))) return r;
    if ((r = dev_alloc(&m.agg, 8 * (frames / 256 + 2)))) return r;
    if ((r = dev_alloc(&m.pre, 8 * (frames / 256 + 2)))) return r;
    if ((r = fws_hip_status(hipMemset(m.agg, 0, 8 * (frames / 256 + 2) * 8)))) return r;
    if ((r = fws_hip_status(hipMemset(m.pre, 0, 8 * (frames / 256 + 2) * 8)))) return r;
    m.cap = frames;
    m.last_epoch = 0;
    return 0;
}

extern "C" {

// Test / tuning hook (not part of the ABI): the decode counters of the last
// decode on ctx (decode_common.h Counter), synchronously. 0 or an error.
__attribute__((visibility("default"))) int fws_internal_decode_counters(fws_gpu_ctx *ctx, uint32_t *out, int n) {
    if (!ctx || !out || n <= 0 || !ctx->dec.counters) return FWS_ERR_INVALID;
    if (n > 64) n = 64;
    return fws_hip_status(hipMemcpy(out, ctx->dec.counters, (size_t)n * 4, hipMemcpyDeviceToHost));
}

// Test hook (not part of the ABI): the last descriptor plan's fws_plan_mode
// words (byte_space, s0, first_po, last_pe, n_units), synchronously.
__attribute__((visibility("default"))) int fws_internal_plan_mode(fws_gpu_ctx *ctx, uint64_t *out5) {
    if (!ctx || !out5 || !ctx->plan.mode) return FWS_ERR_INVALID;
    return fws_hip_status(hipMemcpy(out5, ctx->plan.mode, 5 * 8, hipMemcpyDeviceToHost));
}

// Timing hook (not part of the ABI; tools/msg_bench.py): the parse of
// fws_gpu_decode_stream / fws_gpu_decode_messages alone -- scan + resolve into
// dev_frames / *dev_result, nothing unmasked.
__attribute__((visibility("default"))) int fws_internal_decode_parse(fws_gpu_ctx *ctx, const void *dev_wire,
                                                                     uint64_t len, fws_frame_info *dev_frames,
                                                                     uint32_t cap, fws_decode_result *dev_result,
                                                                     void *stream) {
    if (!ctx || !dev_result || (len && !dev_wire) || (cap && !dev_frames) || ((uintptr_t)dev_wire & 15u))
        return FWS_ERR_INVALID;
    int r;
    if ((r = fws_hip_status(hipSetDevice(ctx->device))) || (r = fws_decode_prepare(ctx, len, cap, false))) return r;
    return fws_launch_decode(ctx, (uint8_t *)const_cast<void *>(dev_wire), len, dev_frames, cap, dev_result, nullptr,
                             (hipStream_t)stream);
}

int fws_gpu_abi_version(void) { return FWS_GPU_ABI_VERSION; }

int fws_gpu_device_count(int *count) {
    if (!count) return FWS_ERR_INVALID;
    *count = 0;
    hipError_t e = hipGetDeviceCount(count);
    if (e == hipErrorNoDevice) { *count = 0; return 0; }
    return fws_hip_status(e);
}

int fws_gpu_ctx_create(int device, fws_gpu_ctx **out) {
    if (!out) return FWS_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    int r = fws_gpu_device_count(&n);
    if (r) return r;
    if (device < 0 || device >= n) return FWS_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if ((r = fws_hip_status(hipGetDeviceProperties(&prop, device)))) return r;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return FWS_ERR_NO_DEVICE;
    if ((r = fws_hip_status(hipSetDevice(device)))) return r;
    fws_gpu_ctx *c = new fws_gpu_ctx();
    c->device = device;
    *out = c;
    return 0;
}

void fws_gpu_ctx_destroy(fws_gpu_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    fws_rx_service_destroy(ctx->svc);    // its grid drained before the buffers it names go
    ctx->svc = nullptr;
    free_plan(ctx->plan);
    dev_free(ctx->any_q);
    dev_free(ctx->any_cnt);
    fws_decode_ws &d = ctx->dec;
    dev_free(d.tile_count);
    dev_free(d.cnt_base);
    dev_free(d.stage_info);
    dev_free(d.spill_info);
    dev_free(d.tile_spill);
    dev_free(d.scan_dummy);
    dev_free(d.nres);
    dev_free(d.tails);
    dev_free(d.gnx);
    dev_free(d.tpk);
    dev_free(d.tmark);
    dev_free(d.comp);
    dev_free(d.st_nodes);
    dev_free(d.st_n);
    dev_free(d.st_nt);
    dev_free(d.st_entry);
    dev_free(d.st_fbase);
    dev_free(d.bg_nx);
    dev_free(d.bg_wt);
    dev_free(d.bg_lref);
    dev_free(d.bg_ptr);
    dev_free(d.bg_sc);
    dev_free(d.bg_mark);
    dev_free(ctx->seam);
    dev_free(ctx->msg.descs);
    dev_free(ctx->msg.ctl_off);
    dev_free(ctx->msg.agg);
    dev_free(ctx->msg.pre);
    dev_free(ctx->msg.cnext);
    delete ctx;
}

int fws_gpu_ctx_reserve(fws_gpu_ctx *ctx, uint64_t max_frames, uint64_t max_stream_bytes) {
    if (!ctx) return FWS_ERR_INVALID;
    int r = fws_hip_status(hipSetDevice(ctx->device));
    if (r) return r;
    // chunks <= bytes / 16 + 2 per frame; units = chunks / 256
    const uint64_t units = (max_stream_bytes / 16 + 2 * max_frames) / 256 + 2;
    if ((r = fws_ctx_ensure_plan(ctx, max_frames, units))) return r;
    // fws_gpu_decode_messages after a reservation never allocates: its parse's
    // workspace and the message planner's are sized here too
    const uint32_t fcap = max_frames < 0xFFFFFFFFull ? (uint32_t)max_frames : 0xFFFFFFFFu;
    if ((r = fws_decode_ensure(ctx, max_stream_bytes, fcap))) return r;
    if ((r = fws_ctx_ensure_msg(ctx, max_frames))) return r;
    if (max_stream_bytes > ctx->cap_stream) ctx->cap_stream = max_stream_bytes;
    return fws_ctx_ensure_seam(ctx, ctx->cap_stream);
}


int fws_gpu_mask(void *dev_ptr, uint64_t n, uint32_t key, void *stream) {
    if (n && !dev_ptr) return FWS_ERR_INVALID;
    return fws_launch_mask_single(dev_ptr, n, key, 0u, (hipStream_t)stream);
}

int fws_gpu_unmask_plan(fws_gpu_ctx *ctx, const void *dev_base, const fws_frame_desc *dev_descs,
                        uint32_t n, void *stream) {
    if (!ctx || (n && (!dev_base || !dev_descs))) return FWS_ERR_INVALID;
    if (n == 0) return 0;
    if (ctx->cap_stream == 0 || n > ctx->cap_frames) return FWS_ERR_CAPACITY;
    if (int r = fws_hip_status(hipSetDevice(ctx->device))) return r;
    return fws_launch_plan((const uint8_t *)dev_base, dev_descs, n, nullptr, ctx->plan, (hipStream_t)stream);
}

int fws_gpu_unmask_run(fws_gpu_ctx *ctx, void *dev_base, const fws_frame_desc *dev_descs,
                       uint32_t n, void *stream) {
    if (!ctx || (n && (!dev_base || !dev_descs))) return FWS_ERR_INVALID;
    if (n == 0) return 0;
    if (ctx->cap_stream == 0 || n > ctx->cap_frames) return FWS_ERR_CAPACITY;
    if (int r = fws_hip_status(hipSetDevice(ctx->device))) return r;
    // the grid is sized from the reservation; a larger batch is still covered in
    // full (grid-stride loop, unit owners past the map's capacity are searched)
    const uint64_t max_chunks = ctx->cap_stream / 16 + 2ull * n;
    return fws_launch_unmask((uint8_t *)dev_base, dev_descs, n, nullptr, ctx->plan, max_chunks,
                             (hipStream_t)stream);
}

int fws_gpu_unmask_batch(fws_gpu_ctx *ctx, void *dev_base, const fws_frame_desc *dev_descs,
                         uint32_t n, void *stream) {
    if (fws_unmask_any_on()) {
        // one launch, descriptor-major (+ the queued pieces of regions over 64 KiB):
        // no plan; the same arguments and capacity checks as the planned form
        if (!ctx || (n && (!dev_base || !dev_descs))) return FWS_ERR_INVALID;
        if (n == 0) return 0;
        if (ctx->cap_stream == 0 || n > ctx->cap_frames) return FWS_ERR_CAPACITY;
        int r;
        if ((r = fws_hip_status(hipSetDevice(ctx->device))) || (r = fws_ctx_ensure_any(ctx))) return r;
        const uint32_t k = ctx->any_parity;
        ctx->any_parity ^= 1u;
        const uint32_t pg = ctx->any_qcap / 4u + 1u;
        return fws_launch_unmask_any((uint8_t *)dev_base, dev_descs, n, ctx->any_q, ctx->any_qcap, ctx->any_cnt + k,
                                     ctx->any_cnt + (k ^ 1u), pg < 2048u ? pg : 2048u, (hipStream_t)stream);
    }
    int r = fws_gpu_unmask_plan(ctx, dev_base, dev_descs, n, stream);
    if (r) return r;
    return fws_gpu_unmask_run(ctx, dev_base, dev_descs, n, stream);
}

}  // extern "C"

int fws_ctx_ensure_any(fws_gpu_ctx *ctx) {
    // pieces come from regions over 64 KiB: at most the reserved span / 64 KiB of
    // them (a batch past the reservation has its waves do their own pieces)
    const uint64_t want = ctx->cap_stream / (64u * 1024u) + 64u;
    const uint32_t cap = (uint32_t)(want < 0x7FFFFFFFull ? want : 0x7FFFFFFFull);
    if (ctx->any_q && ctx->any_qcap >= cap) return 0;
    hipError_t e = hipSuccess;
    if (ctx->any_q) {
        if ((e = hipDeviceSynchronize()) != hipSuccess) return fws_hip_status(e);   // (a regrowth: rare)
        (void)hipFree(ctx->any_q);
        ctx->any_q = nullptr;
    }
    if (!ctx->any_cnt) {
        if ((e = hipMalloc((void **)&ctx->any_cnt, 2 * sizeof(uint32_t))) != hipSuccess) return fws_hip_status(e);
        if ((e = hipMemset(ctx->any_cnt, 0, 2 * sizeof(uint32_t))) != hipSuccess) return fws_hip_status(e);
        ctx->any_parity = 0;
    }
    if ((e = hipMalloc((void **)&ctx->any_q, (uint64_t)cap * sizeof(uint64_t))) != hipSuccess) return fws_hip_status(e);
    ctx->any_qcap = cap;
    return 0;
}

extern "C" {

int fws_gpu_check_sorted(fws_gpu_ctx *ctx, const fws_frame_desc *dev_descs, uint32_t n, uint32_t *dev_bad,
                         void *stream) {
    if (!ctx || !dev_bad || (n && !dev_descs)) return FWS_ERR_INVALID;
    int r;
    if ((r = fws_hip_status(hipSetDevice(ctx->device)))) return r;
    return fws_launch_check_sorted(dev_descs, n, dev_bad, (hipStream_t)stream);
}

// FWS_CHECK_SORTED=1 in the environment: the sorted entry points check the
// contract first and refuse (FWS_ERR_INVALID, nothing written) a violating
// batch; this synchronises the stream (a debug mode, not for timing)
static int check_sorted_debug(fws_gpu_ctx *ctx, const fws_frame_desc *d, uint32_t n, hipStream_t s) {
    static const bool on = [] {
        const char *v = getenv("FWS_CHECK_SORTED");
        return v && v[0] && v[0] != '0';
    }();
    if (!on) return 0;
    uint32_t *bad = nullptr, h = 0;
    hipError_t e = hipMalloc((void **)&bad, sizeof(uint32_t));
    if (e != hipSuccess) return fws_hip_status(e);
    int r = fws_launch_check_sorted(d, n, bad, s);
    if (r == 0 && (e = hipMemcpyAsync(&h, bad, sizeof(h), hipMemcpyDeviceToHost, s)) != hipSuccess) r = fws_hip_status(e);
    if (r == 0 && (e = hipStreamSynchronize(s)) != hipSuccess) r = fws_hip_status(e);
    (void)hipFree(bad);
    if (r) return r;
    return h == 0xFFFFFFFFu ? 0 : FWS_ERR_INVALID;
}

int fws_gpu_unmask_sorted(fws_gpu_ctx *ctx, void *dev_base, const fws_frame_desc *dev_descs, uint32_t n,
                          void *stream) {
    if (!ctx || (n && (!dev_base || !dev_descs))) return FWS_ERR_INVALID;
    if (n == 0) return 0;
    int r;
    if ((r = fws_hip_status(hipSetDevice(ctx->device)))) return r;
    if ((r = check_sorted_debug(ctx, dev_descs, n, (hipStream_t)stream))) return r;
    // the grid only bounds the grid-stride loop: every unit of the span is visited at any grid
    const uint64_t span = ctx->cap_stream ? ctx->cap_stream : 4096ull * n;
    return fws_launch_unmask_sorted((uint8_t *)dev_base, dev_descs, n, span, (hipStream_t)stream);
}

int fws_gpu_unmask_sorted_utf8(fws_gpu_ctx *ctx, void *dev_base, const fws_frame_desc *dev_descs, uint32_t n,
                               uint8_t *dev_ok, void *stream) {
    if (!ctx || (n && (!dev_base || !dev_descs || !dev_ok))) return FWS_ERR_INVALID;
    if (n == 0) return 0;
    int r;
    if ((r = fws_hip_status(hipSetDevice(ctx->device)))) return r;
    if ((r = check_sorted_debug(ctx, dev_descs, n, (hipStream_t)stream))) return r;
    // span only sizes the grid (grid-stride: every unit is visited) and the seam
    // reservation; the kernels bound their seam words by ctx->seam_cap, so a batch
    // whose payload span exceeds it stays in bounds
    const uint64_t span = ctx->cap_stream ? ctx->cap_stream : 4096ull * n;
    if ((r = fws_ctx_ensure_seam(ctx, span))) return r;
    return fws_launch_unmask_sorted_utf8((uint8_t *)dev_base, dev_descs, n, span, dev_ok, ctx->seam, ctx->seam_cap,
                                         (hipStream_t)stream);
}

int fws_gpu_unmask_gather(fws_gpu_ctx *ctx, void *dev_dst, const void *dev_src, const fws_frame_desc *dev_descs,
                          uint32_t n, void *stream) {
    if (!ctx || (n && (!dev_dst || !dev_src || !dev_descs))) return FWS_ERR_INVALID;
    if (((uintptr_t)dev_dst & 15u) != 0) return FWS_ERR_INVALID;
    if (n == 0) return 0;
    if (ctx->cap_stream == 0 || n > ctx->cap_frames) return FWS_ERR_CAPACITY;
    if (int r = fws_hip_status(hipSetDevice(ctx->device))) return r;
    return fws_launch_gather((uint8_t *)dev_dst, (const uint8_t *)dev_src, dev_descs, n, ctx->plan, ctx->cap_stream,
                             (hipStream_t)stream);
}

int fws_gpu_validate_utf8(fws_gpu_ctx *ctx, const void *dev_base, const fws_frame_desc *dev_descs, uint32_t n,
                          uint8_t *dev_ok, void *stream) {
    if (!ctx || (n && (!dev_base || !dev_descs || !dev_ok))) return FWS_ERR_INVALID;
    if (int r = fws_hip_status(hipSetDevice(ctx->device))) return r;
    return fws_launch_utf8_descs((const uint8_t *)dev_base, dev_descs, n, dev_ok, (hipStream_t)stream);
}

int fws_gpu_decode_stream(fws_gpu_ctx *ctx, void *dev_wire, uint64_t len, fws_frame_info *dev_frames,
                          uint32_t cap, fws_decode_result *dev_result, uint8_t *dev_utf8_ok, void *stream) {
    if (!ctx || !dev_result || (len && !dev_wire) || (cap && !dev_frames)) return FWS_ERR_INVALID;
    if (((uintptr_t)dev_wire & 15u) != 0) return FWS_ERR_INVALID;   // tiles are staged with 16-B loads
    hipStream_t s = (hipStream_t)stream;
    int r;
    if ((r = fws_hip_status(hipSetDevice(ctx->device)))) return r;
    if (fws_resolve_mode() == 2 && len <= kSmallMax && !dev_utf8_ok) {
        // test hook: the RX session's one-launch small-read decode, with its
        // fallback taken synchronously as rx_session.cpp does
        if ((r = fws_launch_decode_small((uint8_t *)dev_wire, len, dev_frames, cap, dev_result, s))) return r;
        int32_t st = 0;
        if ((r = fws_hip_status(hipMemcpyAsync(&st, dev_result, 4, hipMemcpyDeviceToHost, s)))) return r;
        if ((r = fws_hip_status(hipStreamSynchronize(s)))) return r;
        if (st != FWS_SMALL_DECLINED) return 0;
    }
    if ((r = fws_decode_prepare(ctx, len, cap, dev_utf8_ok != nullptr))) return r;
    if ((r = fws_launch_decode(ctx, (uint8_t *)dev_wire, len, dev_frames, cap, dev_result, dev_utf8_ok, s)))
        return r;
    return fws_decode_unmask(ctx, (uint8_t *)dev_wire, len, dev_frames, cap, dev_utf8_ok, s);
}

}  // extern "C"

// fws_gpu_decode_messages (carry == null) and fws_gpu_decode_messages_carry: one
// launch sequence; with a carry the planner starts from it, every byte / entry
// overflow denies the gather and the control copy too, and the UTF-8 kernel --
// always launched then, it owns *carry -- rewrites it.
static int decode_messages(fws_gpu_ctx *ctx, const void *dev_wire, uint64_t len, fws_frame_info *dev_frames,
                           uint32_t cap, fws_msg_info *dev_msgs, uint32_t msg_cap, void *dev_dst, uint64_t dst_cap,
                           void *dev_ctl, uint64_t ctl_cap, fws_decode_result *dev_result,
                           fws_msg_result *dev_msg_result, fws_msg_carry *carry, void *stream) {
    if (!ctx || !dev_result || !dev_msg_result || (len && !dev_wire) || (cap && !dev_frames) ||
        (msg_cap && !dev_msgs) || (dst_cap && !dev_dst) || (ctl_cap && !dev_ctl))
        return FWS_ERR_INVALID;
    if ((((uintptr_t)dev_wire | (uintptr_t)dev_dst) & 15u) != 0) return FWS_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    // the parse never writes the wire (k_scan and the resolve read it); its launchers
    // share fws_gpu_decode_stream's pointer type
    uint8_t *const wire = (uint8_t *)const_cast<void *>(dev_wire);
    int r;
    if ((r = fws_hip_status(hipSetDevice(ctx->device)))) return r;
    if ((r = fws_decode_prepare(ctx, len, cap, false)) || (r = fws_ctx_ensure_msg(ctx, cap))) return r;
    // Captured into a graph, the call is replayed with the arguments of this one
    // launch sequence: the counter set and the look-back epochs that eager calls
    // alternate / advance on the host are then the same at every replay. So a
    // captured call records the two resets itself (memset nodes on the same
    // chain): its counter set, and the look-back words the planner and the gather
    // plan tag.
    bool capturing = false;
    if (s) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if ((r = fws_hip_status(hipStreamIsCapturing(s, &cs)))) return r;
        capturing = cs == hipStreamCaptureStatusActive;
    }
    if (capturing) {
        ctx->dec.cnt_dirty = true;
        if ((r = fws_hip_status(hipMemsetAsync(ctx->plan.status, 0, ctx->plan.status_cap * 8, s)))) return r;
    }
    r = fws_launch_decode(ctx, wire, len, dev_frames, cap, dev_result, nullptr, s);
    if (capturing) ctx->dec.cnt_dirty = true;          // the other set is zeroed only when the graph runs
    if (r) return r;
    // the resolve left the device frame count; its stream-space unmask plan in
    // ctx->plan is not used (no in-place unmask follows): the planner's look-back
    // and the gather plan take that workspace over
    const uint32_t *n_dev = ctx->dec.counters + kDecodeFramesCounter;
    if ((r = fws_launch_msg_plan(ctx, len, dev_frames, cap, n_dev, dev_result, dev_msgs, msg_cap, dst_cap, ctl_cap,
                                 dev_msg_result, capturing, s, carry)))
        return r;
    const fws_msg_carry_next *cn = carry ? ctx->msg.cnext : nullptr;
    const uint32_t *deny = carry ? &ctx->msg.cnext->deny : nullptr;
    // unmask + compaction in one pass: the gather over the planner's cap descriptors
    // (the data frames' payloads with their keys, then zero-length regions)
    if (cap && dst_cap) {
        const uint64_t max_bytes = len < dst_cap ? len : dst_cap;
        if ((r = fws_launch_gather((uint8_t *)dev_dst, wire, ctx->msg.descs, cap, ctx->plan, max_bytes, s, dst_cap,
                                   deny)))
            return r;
    }
    if (ctl_cap && (r = fws_launch_msg_ctl(ctx, wire, dev_frames, cap, n_dev, dev_msg_result, (uint8_t *)dev_ctl,
                                           ctl_cap, s, deny)))
        return r;
    if (carry || (cap && dst_cap))
        return fws_launch_utf8_msgs((const uint8_t *)dev_dst, dev_msgs, msg_cap, dev_msg_result, dst_cap, s, cn, carry);
    return 0;
}

extern "C" {

int fws_gpu_decode_messages(fws_gpu_ctx *ctx, const void *dev_wire, uint64_t len, fws_frame_info *dev_frames,
                            uint32_t cap, fws_msg_info *dev_msgs, uint32_t msg_cap, void *dev_dst, uint64_t dst_cap,
                            void *dev_ctl, uint64_t ctl_cap, fws_decode_result *dev_result,
                            fws_msg_result *dev_msg_result, void *stream) {
    return decode_messages(ctx, dev_wire, len, dev_frames, cap, dev_msgs, msg_cap, dev_dst, dst_cap, dev_ctl, ctl_cap,
                           dev_result, dev_msg_result, nullptr, stream);
}

int fws_gpu_decode_messages_carry(fws_gpu_ctx *ctx, const void *dev_wire, uint64_t len, fws_frame_info *dev_frames,
                                  uint32_t cap, fws_msg_info *dev_msgs, uint32_t msg_cap, void *dev_dst,
                                  uint64_t dst_cap, void *dev_ctl, uint64_t ctl_cap, fws_decode_result *dev_result,
                                  fws_msg_result *dev_msg_result, fws_msg_carry *dev_carry, void *stream) {
    if (!dev_carry) return FWS_ERR_INVALID;
    return decode_messages(ctx, dev_wire, len, dev_frames, cap, dev_msgs, msg_cap, dev_dst, dst_cap, dev_ctl, ctl_cap,
                           dev_result, dev_msg_result, dev_carry, stream);
}

int fws_gpu_decode_messages_multi(fws_gpu_ctx *ctx, const void *dev_wire, const fws_msg_read *dev_reads, uint32_t n,
                                  uint32_t max_len, fws_frame_info *dev_frames, fws_msg_info *dev_msgs, void *dev_dst,
                                  void *dev_ctl, fws_decode_result *dev_results, fws_msg_result *dev_msg_results,
                                  fws_msg_carry *dev_carries, uint32_t n_conns, void *stream) {
    if (n == 0) return 0;
    if (!ctx || !dev_wire || !dev_reads || !dev_frames || !dev_msgs || !dev_dst || !dev_ctl || !dev_results ||
        !dev_msg_results || !dev_carries)
        return FWS_ERR_INVALID;
    if ((((uintptr_t)dev_wire | (uintptr_t)dev_dst) & 15u) != 0) return FWS_ERR_INVALID;
    if (max_len < 1u || max_len > FWS_MSG_MULTI_MAX_READ) return FWS_ERR_INVALID;
    if (int r = fws_hip_status(hipSetDevice(ctx->device))) return r;
    return fws_launch_msg_multi((const uint8_t *)dev_wire, dev_reads, n, max_len, dev_frames, dev_msgs,
                                (uint8_t *)dev_dst, (uint8_t *)dev_ctl, dev_results, dev_msg_results, dev_carries,
                                n_conns, (hipStream_t)stream);
}

// both roles of the flow decode: the checks, then the launch
static int decode_messages_flow(fws_gpu_ctx *ctx, const void *dev_wire, const fws_msg_read *dev_reads, uint32_t n,
                                uint32_t max_len, fws_frame_info *dev_frames, fws_msg_info *dev_msgs, void *dev_dst,
                                void *dev_ctl, fws_decode_result *dev_results, fws_msg_result *dev_msg_results,
                                fws_msg_flow *dev_flows, uint32_t n_conns, void *stream, bool client) {
    if (n == 0) return 0;
    if (!ctx || !dev_wire || !dev_reads || !dev_frames || !dev_msgs || !dev_dst || !dev_ctl || !dev_results ||
        !dev_msg_results || !dev_flows)
        return FWS_ERR_INVALID;
    if ((((uintptr_t)dev_wire | (uintptr_t)dev_dst) & 15u) != 0) return FWS_ERR_INVALID;
    if (max_len < 1u || max_len > FWS_MSG_MULTI_MAX_READ) return FWS_ERR_INVALID;
    if (int r = fws_hip_status(hipSetDevice(ctx->device))) return r;
    return fws_launch_msg_flow((const uint8_t *)dev_wire, dev_reads, n, max_len, dev_frames, dev_msgs,
                               (uint8_t *)dev_dst, (uint8_t *)dev_ctl, dev_results, dev_msg_results, dev_flows,
                               n_conns, (hipStream_t)stream, client);
}

int fws_gpu_decode_messages_flow(fws_gpu_ctx *ctx, const void *dev_wire, const fws_msg_read *dev_reads, uint32_t n,
                                 uint32_t max_len, fws_frame_info *dev_frames, fws_msg_info *dev_msgs, void *dev_dst,
                                 void *dev_ctl, fws_decode_result *dev_results, fws_msg_result *dev_msg_results,
                                 fws_msg_flow *dev_flows, uint32_t n_conns, void *stream) {
    return decode_messages_flow(ctx, dev_wire, dev_reads, n, max_len, dev_frames, dev_msgs, dev_dst, dev_ctl,
                                dev_results, dev_msg_results, dev_flows, n_conns, stream, false);
}

int fws_gpu_decode_messages_flow_client(fws_gpu_ctx *ctx, const void *dev_wire, const fws_msg_read *dev_reads,
                                        uint32_t n, uint32_t max_len, fws_frame_info *dev_frames,
                                        fws_msg_info *dev_msgs, void *dev_dst, void *dev_ctl,
                                        fws_decode_result *dev_results, fws_msg_result *dev_msg_results,
                                        fws_msg_flow *dev_flows, uint32_t n_conns, void *stream) {
    return decode_messages_flow(ctx, dev_wire, dev_reads, n, max_len, dev_frames, dev_msgs, dev_dst, dev_ctl,
                                dev_results, dev_msg_results, dev_flows, n_conns, stream, true);
}

int fws_gpu_encode_messages_multi(fws_gpu_ctx *ctx, void *dev_out, const void *dev_src, const fws_tx_send *dev_sends,
                                  uint32_t n, uint32_t max_len, fws_frame_info *dev_frames,
                                  fws_tx_result *dev_results, fws_tx_conn *dev_conns, uint32_t n_conns,
                                  void *stream) {
    if (n == 0) return 0;
    // (dev_frames may be null: a send with frame_cap 0 writes no record)
    if (!ctx || !dev_out || !dev_src || !dev_sends || !dev_results || !dev_conns) return FWS_ERR_INVALID;
    if (((uintptr_t)dev_out & 15u) != 0) return FWS_ERR_INVALID;
    if (max_len < 1u || max_len > FWS_TX_MULTI_MAX_SEND) return FWS_ERR_INVALID;
    if (int r = fws_hip_status(hipSetDevice(ctx->device))) return r;
    return fws_launch_tx_multi((uint8_t *)dev_out, (const uint8_t *)dev_src, dev_sends, n, max_len, dev_frames,
                               dev_results, dev_conns, n_conns, (hipStream_t)stream);
}

// both forms of the reply: the checks, then the launch (dev_keys non-null: client frames)
static int reply_messages_multi(fws_gpu_ctx *ctx, const fws_msg_read *dev_reads, uint32_t n, uint32_t max_len,
                                const fws_msg_info *dev_msgs, const void *dev_dst, const void *dev_ctl,
                                const fws_msg_result *dev_msg_results, const fws_reply_region *dev_regions,
                                void *dev_out, fws_frame_info *dev_frames, fws_tx_result *dev_results,
                                fws_tx_conn *dev_conns, fws_reply_state *dev_states, uint32_t n_conns,
                                uint32_t flags, const uint32_t *dev_keys, void *stream) {
    // (dev_frames may be null: a read with frame_cap 0 writes no record)
    if (!ctx || !dev_reads || !dev_msgs || !dev_dst || !dev_ctl || !dev_msg_results || !dev_regions || !dev_out ||
        !dev_results || !dev_conns || !dev_states)
        return FWS_ERR_INVALID;
    if (((uintptr_t)dev_out & 15u) != 0) return FWS_ERR_INVALID;
    if (max_len < 1u || max_len > FWS_MSG_MULTI_MAX_READ) return FWS_ERR_INVALID;
    if (flags & ~(FWS_REPLY_CONTROL | FWS_REPLY_ECHO)) return FWS_ERR_INVALID;
    if (int r = fws_hip_status(hipSetDevice(ctx->device))) return r;
    if (dev_keys)
        return fws_launch_reply_client(dev_reads, n, max_len, dev_msgs, (const uint8_t *)dev_dst,
                                       (const uint8_t *)dev_ctl, dev_msg_results, dev_regions, (uint8_t *)dev_out,
                                       dev_frames, dev_results, dev_conns, dev_states, n_conns, flags, dev_keys,
                                       (hipStream_t)stream);
    return fws_launch_reply(dev_reads, n, max_len, dev_msgs, (const uint8_t *)dev_dst, (const uint8_t *)dev_ctl,
                            dev_msg_results, dev_regions, (uint8_t *)dev_out, dev_frames, dev_results, dev_conns,
                            dev_states, n_conns, flags, (hipStream_t)stream);
}

int fws_gpu_reply_messages_multi(fws_gpu_ctx *ctx, const fws_msg_read *dev_reads, uint32_t n, uint32_t max_len,
                                 const fws_msg_info *dev_msgs, const void *dev_dst, const void *dev_ctl,
                                 const fws_msg_result *dev_msg_results, const fws_reply_region *dev_regions,
                                 void *dev_out, fws_frame_info *dev_frames, fws_tx_result *dev_results,
                                 fws_tx_conn *dev_conns, fws_reply_state *dev_states, uint32_t n_conns,
                                 uint32_t flags, void *stream) {
    if (n == 0) return 0;
    return reply_messages_multi(ctx, dev_reads, n, max_len, dev_msgs, dev_dst, dev_ctl, dev_msg_results, dev_regions,
                                dev_out, dev_frames, dev_results, dev_conns, dev_states, n_conns, flags, nullptr,
                                stream);
}

int fws_gpu_reply_messages_multi_client(fws_gpu_ctx *ctx, const fws_msg_read *dev_reads, uint32_t n, uint32_t max_len,
                                        const fws_msg_info *dev_msgs, const void *dev_dst, const void *dev_ctl,
                                        const fws_msg_result *dev_msg_results, const fws_reply_region *dev_regions,
                                        void *dev_out, fws_frame_info *dev_frames, fws_tx_result *dev_results,
                                        fws_tx_conn *dev_conns, fws_reply_state *dev_states, uint32_t n_conns,
                                        uint32_t flags, const uint32_t *dev_keys, void *stream) {
    if (n == 0) return 0;
    if (!dev_keys) return FWS_ERR_INVALID;
    return reply_messages_multi(ctx, dev_reads, n, max_len, dev_msgs, dev_dst, dev_ctl, dev_msg_results, dev_regions,
                                dev_out, dev_frames, dev_results, dev_conns, dev_states, n_conns, flags, dev_keys,
                                stream);
}

static int reply_messages_strict(fws_gpu_ctx *ctx, const fws_msg_read *dev_reads, uint32_t n, uint32_t max_len,
                                 const fws_msg_info *dev_msgs, const void *dev_dst, const void *dev_ctl,
                                 const fws_msg_result *dev_msg_results, const void *dev_conn_states,
                                 uint32_t conn_state_stride, uint64_t max_message_bytes,
                                 const fws_reply_region *dev_regions, void *dev_out, fws_frame_info *dev_frames,
                                 fws_tx_result *dev_results, fws_tx_conn *dev_conns, fws_reply_state *dev_states,
                                 uint32_t n_conns, uint32_t flags, const uint32_t *dev_keys, void *stream) {
    // (dev_frames may be null: a read with frame_cap 0 writes no record)
    if (!ctx || !dev_reads || !dev_msgs || !dev_dst || !dev_ctl || !dev_msg_results || !dev_conn_states ||
        !dev_regions || !dev_out || !dev_results || !dev_conns || !dev_states)
        return FWS_ERR_INVALID;
    if (conn_state_stride != sizeof(fws_msg_carry) && conn_state_stride != sizeof(fws_msg_flow)) return FWS_ERR_INVALID;
    if (((uintptr_t)dev_out & 15u) != 0) return FWS_ERR_INVALID;
    if (max_len < 1u || max_len > FWS_MSG_MULTI_MAX_READ) return FWS_ERR_INVALID;
    if (flags & ~(FWS_REPLY_CONTROL | FWS_REPLY_ECHO)) return FWS_ERR_INVALID;
    if (int r = fws_hip_status(hipSetDevice(ctx->device))) return r;
    if (dev_keys)
        return fws_launch_reply_strict_client(dev_reads, n, max_len, dev_msgs, (const uint8_t *)dev_dst,
                                              (const uint8_t *)dev_ctl, dev_msg_results,
                                              (const uint8_t *)dev_conn_states, conn_state_stride, max_message_bytes,
                                              dev_regions, (uint8_t *)dev_out, dev_frames, dev_results, dev_conns,
                                              dev_states, n_conns, flags, dev_keys, (hipStream_t)stream);
    return fws_launch_reply_strict(dev_reads, n, max_len, dev_msgs, (const uint8_t *)dev_dst, (const uint8_t *)dev_ctl,
                                   dev_msg_results, (const uint8_t *)dev_conn_states, conn_state_stride,
                                   max_message_bytes, dev_regions, (uint8_t *)dev_out, dev_frames, dev_results,
                                   dev_conns, dev_states, n_conns, flags, (hipStream_t)stream);
}

int fws_gpu_reply_messages_strict(fws_gpu_ctx *ctx, const fws_msg_read *dev_reads, uint32_t n, uint32_t max_len,
                                  const fws_msg_info *dev_msgs, const void *dev_dst, const void *dev_ctl,
                                  const fws_msg_result *dev_msg_results, const void *dev_conn_states,
                                  uint32_t conn_state_stride, uint64_t max_message_bytes,
                                  const fws_reply_region *dev_regions, void *dev_out, fws_frame_info *dev_frames,
                                  fws_tx_result *dev_results, fws_tx_conn *dev_conns, fws_reply_state *dev_states,
                                  uint32_t n_conns, uint32_t flags, void *stream) {
    if (n == 0) return 0;
    return reply_messages_strict(ctx, dev_reads, n, max_len, dev_msgs, dev_dst, dev_ctl, dev_msg_results,
                                 dev_conn_states, conn_state_stride, max_message_bytes, dev_regions, dev_out,
                                 dev_frames, dev_results, dev_conns, dev_states, n_conns, flags, nullptr, stream);
}

int fws_gpu_reply_messages_strict_client(fws_gpu_ctx *ctx, const fws_msg_read *dev_reads, uint32_t n,
                                         uint32_t max_len, const fws_msg_info *dev_msgs, const void *dev_dst,
                                         const void *dev_ctl, const fws_msg_result *dev_msg_results,
                                         const void *dev_conn_states, uint32_t conn_state_stride,
                                         uint64_t max_message_bytes, const fws_reply_region *dev_regions,
                                         void *dev_out, fws_frame_info *dev_frames, fws_tx_result *dev_results,
                                         fws_tx_conn *dev_conns, fws_reply_state *dev_states, uint32_t n_conns,
                                         uint32_t flags, const uint32_t *dev_keys, void *stream) {
    if (n == 0) return 0;
    if (!dev_keys) return FWS_ERR_INVALID;
    return reply_messages_strict(ctx, dev_reads, n, max_len, dev_msgs, dev_dst, dev_ctl, dev_msg_results,
                                 dev_conn_states, conn_state_stride, max_message_bytes, dev_regions, dev_out,
                                 dev_frames, dev_results, dev_conns, dev_states, n_conns, flags, dev_keys, stream);
}

int fws_gpu_join_messages(fws_gpu_ctx *ctx, const fws_msg_read *dev_reads, uint32_t n, uint32_t max_len,
                          const fws_msg_info *dev_msgs, const void *dev_dst, const fws_msg_result *dev_msg_results,
                          void *dev_store, uint64_t store_stride, fws_join_info *dev_joined,
                          fws_join_result *dev_results, fws_join_state *dev_states, uint32_t n_conns, void *stream) {
    if (n == 0) return 0;
    if (!ctx || !dev_reads || !dev_msgs || !dev_dst || !dev_msg_results || !dev_store || !dev_joined || !dev_results ||
        !dev_states)
        return FWS_ERR_INVALID;
    if ((((uintptr_t)dev_dst | (uintptr_t)dev_store) & 15u) != 0) return FWS_ERR_INVALID;
    if (max_len < 1u || max_len > FWS_MSG_MULTI_MAX_READ) return FWS_ERR_INVALID;
    if (store_stride < 32u || (store_stride & 31u) != 0) return FWS_ERR_INVALID;
    if (int r = fws_hip_status(hipSetDevice(ctx->device))) return r;
    return fws_launch_join(dev_reads, n, max_len, dev_msgs, (const uint8_t *)dev_dst, dev_msg_results,
                           (uint8_t *)dev_store, store_stride, dev_joined, dev_results, dev_states, n_conns,
                           (hipStream_t)stream);
}

int fws_gpu_publish_messages(fws_gpu_ctx *ctx, const fws_join_info *dev_msgs, uint32_t n_msgs, const void *dev_dst,
                             const void *dev_store, const void *dev_ctl, const uint32_t *dev_list, uint32_t n_list,
                             const fws_pub_sub *dev_subs, uint32_t n, uint32_t max_len, void *dev_out,
                             fws_frame_info *dev_frames, fws_tx_result *dev_results, fws_tx_conn *dev_conns,
                             fws_reply_state *dev_states, uint32_t n_conns, void *stream) {
    if (n == 0) return 0;
    // (dev_dst, dev_store and dev_ctl may be null: a record that names a null base refuses its subscriber;
    // dev_frames may be null: a subscriber with frame_cap 0 writes no record)
    if (!ctx || !dev_msgs || !dev_list || !dev_subs || !dev_out || !dev_results || !dev_conns || !dev_states)
        return FWS_ERR_INVALID;
    if (((uintptr_t)dev_out & 15u) != 0) return FWS_ERR_INVALID;
    if (max_len < 1u || max_len > FWS_TX_MULTI_MAX_SEND) return FWS_ERR_INVALID;
    if (int r = fws_hip_status(hipSetDevice(ctx->device))) return r;
    return fws_launch_publish(dev_msgs, n_msgs, (const uint8_t *)dev_dst, (const uint8_t *)dev_store,
                              (const uint8_t *)dev_ctl, dev_list, n_list, dev_subs, n, max_len, (uint8_t *)dev_out,
                              dev_frames, dev_results, dev_conns, dev_states, n_conns, (hipStream_t)stream);
}

}  // extern "C"

int fws_decode_prepare(fws_gpu_ctx *ctx, uint64_t len, uint32_t cap, bool utf8) {
    int r;
    if ((r = fws_decode_ensure(ctx, len, cap))) return r;
    const uint64_t units = (len / 16 + 2ull * cap) / 256 + 2;
    if ((r = fws_ctx_ensure_plan(ctx, cap, units))) return r;
    return utf8 ? fws_ctx_ensure_seam(ctx, len) : 0;
}

int fws_decode_unmask(fws_gpu_ctx *ctx, uint8_t *wire, uint64_t len, fws_frame_info *frames, uint32_t cap,
                      uint8_t *utf8_ok, hipStream_t s) {
    if (cap == 0 || len == 0) return 0;
    // the resolve left the device frame count, the stream-space unmask plan of the
    // decoded frames and (with utf8_ok) each frame's TEXT/FIN/complete preset;
    // the unmask checks UTF-8 while the payload is in registers
    const uint32_t *n_dev = ctx->dec.counters + kDecodeFramesCounter;
    return fws_launch_unmask_stream(wire, len, frames, cap, n_dev, ctx->plan.unit_first, utf8_ok, ctx->seam, s);
}

