/*
 * fws_gpu.h -- C ABI of flashws_amd: the MI355X (gfx950) receive-path frame
 * decode of flashws (RFC 6455 §5.2 header parse + 4-byte-key XOR unmask).
 *
 * Pure C. No HIP or torch types in the signatures: device memory is `void *`,
 * streams are `void *` (a hipStream_t, NULL = the null stream). Every entry
 * point returns an int status (0 = ok, negative = error, table below); none
 * throws, none frees caller memory, none synchronises the stream unless its
 * comment says so.
 *
 * Reference interfaces replaced (paths relative to flashws include/flashws/):
 *   seam 1  fws::WSMaskBytesFast(uint8_t*, size_t, uint32_t)  crypto/ws_mask.h:175-197
 *           -> fws_gpu_mask / fws_gpu_unmask_batch
 *   seam 2  WSocket<D, is_server, tls>::OnRecvData(IOBuffer&) net/w_socket.h:543-769
 *           (its ParseFrameHdr net/w_socket.h:435-524 and RX state :223-245)
 *           -> fws_gpu_decode_stream (device-resident batch)
 *           -> fws_rx_session_* (host buffers, same on_read() event contract)
 * The reference-side binding a maintainer adds is in INTEGRATION.md.
 */
#ifndef FWS_GPU_H
#define FWS_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FWS_GPU_ABI_VERSION 1

/* ---- status codes ------------------------------------------------------
 * Protocol errors keep the reference's ParseFrameHdr return values
 * (w_socket.h:451-521) so callers can forward them unchanged to
 * WSServerSocket's Close(WS_ABNORMAL_CLOSE, ...) (ws_server_socket.h:176-181). */
enum {
    FWS_OK = 0,
    FWS_ERR_RSV = -1,           /* RSV1-3 set                 w_socket.h:466-470 */
    FWS_ERR_TOO_LARGE = -2,     /* payload_len > 2^32         w_socket.h:493-498 */
    FWS_ERR_NOT_MASKED = -3,    /* server RX, MASK bit clear  w_socket.h:513-515 */
    FWS_ERR_MASKED = -4,        /* client RX, MASK bit set    w_socket.h:518-521 */
    FWS_ERR_OPCODE = -9,        /* opcode not 0-2/8-10        w_socket.h:451-454 */
    FWS_ERR_CONTROL_FRAME = -10,/* host RX session: control frame with payload > 125 B
                                   (RFC 6455 §5.5). The reference does not check
                                   (only a debug FWS_ASSERT, w_socket.h:654) and overflows
                                   its control buffer; the session refuses the frame.
                                   fws_gpu_decode_messages: the same, and a control frame
                                   with FIN = 0. */
    FWS_ERR_SEQUENCE = -11,     /* fws_gpu_decode_messages: a continuation frame with no message
                                   open, or a TEXT / BIN frame while one is open (RFC 6455
                                   §5.4). The reference does not check. */
    FWS_ERR_CAPACITY = -20,     /* an output array is too small (count still reported) */
    FWS_ERR_INVALID = -21,      /* bad argument / not initialised */
    FWS_ERR_NO_DEVICE = -22,    /* no gfx950 device visible */
    FWS_ERR_INTERNAL = -23,     /* device-side failure (decode grid barrier timed out) */
    FWS_ERR_DECLINED = -24,     /* fws_gpu_decode_messages_multi, per read: the read is outside the
                                   one-launch form's limits; run fws_gpu_decode_messages_carry on it */
    FWS_ERR_HIP_BASE = -1000    /* -1000 - hipError_t */
};

/* ---- descriptor-mode unmask --------------------------------------------
 * One payload region to unmask in place. Byte i of the region is XORed with
 * key byte ((phase + i) & 3), key = the 4 wire key bytes loaded as a native
 * little-endian uint32 (w_socket.h:504; ws_mask.h:17-28). Continuing a frame
 * at payload offset k is phase = k & 3, the same as the reference's
 * RotateR(key, 8 * (k & 3)) (w_socket.h:756-759). Regions of one batch must
 * not overlap; they may be in any order and any alignment. */
typedef struct fws_frame_desc {
    uint64_t payload_off;   /* byte offset from the batch's device base */
    uint64_t payload_len;   /* bytes to unmask (0 allowed) */
    uint32_t key;
    uint32_t phase;         /* 0..3 */
} fws_frame_desc;           /* 24 bytes */

/* ---- stream decode output ------------------------------------------------
 * One parsed frame of a server-side (client-masked) byte stream. */
typedef struct fws_frame_info {
    uint64_t hdr_off;       /* offset of the frame's first header byte */
    uint64_t payload_len;   /* length field from the header (w_socket.h:473-492) */
    uint32_t key;           /* mask key, native LE u32 of the wire bytes */
    uint8_t opcode;         /* raw opcode of this frame (0 = continuation) */
    uint8_t fin;
    uint8_t hdr_len;        /* 6, 8 or 14 */
    uint8_t flags;          /* FWS_FRAME_TRUNCATED: payload runs past the stream end */
} fws_frame_info;           /* 24 bytes */

#define FWS_FRAME_TRUNCATED 1u

/* Result of one fws_gpu_decode_stream call (written to device memory). */
typedef struct fws_decode_result {
    int32_t status;         /* FWS_OK or the first protocol error on the stream */
    uint32_t n_frames;      /* frames parsed (complete headers), also past capacity */
    uint64_t consumed;      /* bytes consumed: end of last frame part (== len unless a
                               partial header remains, or an error stopped the decode) */
    uint64_t err_off;       /* offset of the failing header when status < 0 */
    uint64_t carry_unread;  /* payload bytes of the last frame still to come */
    uint32_t carry_hdr_len; /* bytes of an incomplete trailing header (<= 13) */
    uint32_t n_survivors;   /* diagnostics: speculative header candidates kept */
} fws_decode_result;        /* 40 bytes */

typedef struct fws_gpu_ctx fws_gpu_ctx;

int fws_gpu_abi_version(void);
int fws_gpu_device_count(int *count);

/* A context owns the device workspace of one device and is used from one
 * host thread at a time (one context per stream/thread; the reference is one
 * FLoop per thread, floop.h:331-345). */
int fws_gpu_ctx_create(int device, fws_gpu_ctx **out);
void fws_gpu_ctx_destroy(fws_gpu_ctx *ctx);
/* Pre-size the workspace so later calls never allocate (hipGraph-capturable). */
int fws_gpu_ctx_reserve(fws_gpu_ctx *ctx, uint64_t max_frames, uint64_t max_stream_bytes);
/* Persistent receive decode (r05): with workers > 0, the small reads of the
 * context's fws_rx_session / fws_rx_mux calls (reads of <= 128 KiB in pinned
 * or registered host memory, the per-read and per-loop-step hot path of
 * OnRecvData, w_socket.h:543-769) are decoded by a resident grid of `workers`
 * workgroups (+ one poller) that the context launches on first use and that
 * exits by itself after ~250 us without a read -- no kernel launch per read
 * while reads keep coming. 0 (the default) = a launch per read. The grid holds
 * `workers` CUs' LDS and one hardware queue while it is resident. On a device
 * with a large BAR the grid polls a mailbox in device memory that the CPU
 * writes, and a session read of <= 16 KiB is copied there by the CPU with its
 * doorbell (push mode; FWS_RX_PUSH=0 in the environment keeps every read a
 * device-side pull over PCIe). Results are the same either way. */
int fws_gpu_ctx_set_rx_persistent(fws_gpu_ctx *ctx, uint32_t workers);

/* seam 1 -- device twin of WSMaskBytesFast (ws_mask.h:175): XOR n bytes at
 * dev_ptr with key, in place, on `stream`. Any alignment, any n. */
int fws_gpu_mask(void *dev_ptr, uint64_t n, uint32_t key, void *stream);

/* Descriptor-mode batch unmask: every region of dev_descs[0..n) (device
 * memory) inside dev_base is unmasked in place. Load-balanced over 4 KiB
 * units, so one launch covers any mix of frame sizes. Regions must not
 * overlap; any order is accepted. When they are sorted by offset (a batch cut
 * from a wire stream) the run works in byte space: non-payload bytes that
 * share a 16-byte aligned chunk with payload bytes, between the batch's first
 * and last payload byte, are written back with their own value (no other
 * writer may change them during the call); bytes outside that span are never
 * written. A permuted batch is planned in chunk space (C2 permuted: 0.142 ms
 * against 0.091 sorted). */
int fws_gpu_unmask_batch(fws_gpu_ctx *ctx, void *dev_base, const fws_frame_desc *dev_descs,
                         uint32_t n, void *stream);

/* One-launch batch unmask for descriptors sorted by payload_off with
 * non-overlapping regions (payload_off_i + payload_len_i <= payload_off_i+1),
 * as a batch cut from a wire stream or fws_gpu_decode_stream's frame list
 * always is. Same result and the same byte-space write rule as
 * fws_gpu_unmask_batch, without its plan launch: each 4 KiB unit finds its
 * frames itself (interpolation guess, binary search on a miss). Unsorted or
 * overlapping descriptors are a contract violation: results are undefined
 * inside [first payload, last payload end), nothing outside it is written.
 * Replaces the per-frame WSMaskBytesFast calls (ws_mask.h:175) of
 * OnRecvData's frame loop (w_socket.h:586,614) for a whole batch. */
int fws_gpu_unmask_sorted(fws_gpu_ctx *ctx, void *dev_base, const fws_frame_desc *dev_descs,
                          uint32_t n, void *stream);

/* The sortedness contract of fws_gpu_unmask_sorted(_utf8), checked on the
 * device in one launch: *dev_bad (a device word) becomes the first i with
 * payload_off_i + payload_len_i > payload_off_i+1 (or an overflowing end), or
 * 0xFFFFFFFF when the batch is sorted and disjoint. With FWS_CHECK_SORTED=1
 * in the environment the sorted entry points run this check first and refuse
 * a violating batch with FWS_ERR_INVALID, writing nothing (a debug mode: it
 * synchronises the stream). */
int fws_gpu_check_sorted(fws_gpu_ctx *ctx, const fws_frame_desc *dev_descs, uint32_t n, uint32_t *dev_bad,
                         void *stream);

/* fws_gpu_unmask_sorted plus per-region UTF-8 validation of the unmasked
 * payloads in the same pass (BASELINE config 5 in descriptor mode):
 * dev_ok[i] = 1 iff region i is well-formed UTF-8 (Unicode Table 3-7), the
 * same flags as fws_gpu_unmask_sorted followed by fws_gpu_validate_utf8.
 * Same sortedness contract as fws_gpu_unmask_sorted. */
int fws_gpu_unmask_sorted_utf8(fws_gpu_ctx *ctx, void *dev_base, const fws_frame_desc *dev_descs, uint32_t n,
                               uint8_t *dev_ok, void *stream);

/* The two halves of fws_gpu_unmask_batch, for callers that reuse one plan
 * (same descriptors) across buffers: _plan builds the chunk plan of the
 * descriptors in ctx, _run unmasks with the last plan built in ctx. */
int fws_gpu_unmask_plan(fws_gpu_ctx *ctx, const void *dev_base, const fws_frame_desc *dev_descs,
                        uint32_t n, void *stream);
int fws_gpu_unmask_run(fws_gpu_ctx *ctx, void *dev_base, const fws_frame_desc *dev_descs,
                       uint32_t n, void *stream);

/* Same, out of place: dst[dst_off_i ..] = src[payload_off_i ..] ^ key, with
 * dst_off = exclusive prefix sum of payload_len (message reassembly, C4). */
int fws_gpu_unmask_gather(fws_gpu_ctx *ctx, void *dev_dst, const void *dev_src,
                          const fws_frame_desc *dev_descs, uint32_t n, void *stream);

/* seam 2 (device-resident) -- fused header parse + unmask of a server-side
 * wire stream dev_wire[0..len) that starts at a frame header. Payloads are
 * unmasked in place; frames are listed in dev_frames (capacity cap) and the
 * outcome in *dev_result (device memory). Semantics are OnRecvData's on one
 * buffer: decoding stops at the first protocol error (frames before it are
 * still unmasked), a truncated last payload is unmasked as far as present, an
 * incomplete trailing header is left for the next call. If dev_utf8_ok is
 * non-NULL, byte i of it is set to 1 iff frame i is TEXT (opcode 1), FIN,
 * complete, and its unmasked payload is well-formed UTF-8 (else 0). */
int fws_gpu_decode_stream(fws_gpu_ctx *ctx, void *dev_wire, uint64_t len,
                          fws_frame_info *dev_frames, uint32_t cap,
                          fws_decode_result *dev_result, uint8_t *dev_utf8_ok, void *stream);

/* ---- stream decode into messages ------------------------------------------
 * What a WebSocket application consumes: whole messages, reassembled from
 * their fragments (RFC 6455 §5.4), TEXT ones checked for UTF-8 (§8.1), control
 * frames apart from the data they interrupt (§5.5). One entry per completed
 * unit, in completion order -- the order an application's callback would see:
 * a data message at its FIN frame, a control frame at its own position (a PING
 * between two fragments comes before the message it interrupts). */
typedef struct fws_msg_info {
    uint64_t off;           /* data: offset in dev_dst; control: offset in dev_ctl */
    uint64_t len;
    uint32_t first_frame;   /* index into dev_frames */
    uint32_t last_frame;
    uint32_t n_data_frames; /* fragments of the message (control: 1) */
    uint8_t opcode;         /* 1 TEXT, 2 BIN, 8 CLOSE, 9 PING, 10 PONG */
    uint8_t utf8_ok;        /* TEXT message: 1 iff the reassembled bytes are well-formed UTF-8; else 0 */
    uint8_t flags;          /* 0; fws_gpu_decode_messages_carry: FWS_MSG_CONTINUED */
    uint8_t pad;
} fws_msg_info;            /* 32 bytes */

typedef struct fws_msg_result {
    int32_t status;         /* see fws_gpu_decode_messages */
    uint32_t n_msgs;        /* entries produced, also past msg_cap */
    uint32_t err_frame;     /* frame index of a sequencing error (else 0xFFFFFFFF) */
    uint32_t open_first_frame; /* first frame of the unfinished last message, 0xFFFFFFFF if none */
    uint32_t open_opcode;   /* 1 / 2, 0 if none */
    uint32_t n_data_frames; /* data frames placed in dev_dst */
    uint64_t data_bytes;    /* bytes placed in dev_dst, open message included */
    uint64_t ctl_bytes;     /* bytes placed in dev_ctl */
    uint64_t open_off;      /* dev_dst offset and length of the open message's present bytes */
    uint64_t open_len;
    uint64_t resume_off;    /* wire offset to resubmit from: the open message's first header,
                               else the end of the last frame processed */
} fws_msg_result;           /* 64 bytes */

/* fws_gpu_decode_stream's parse of a server-side wire stream dev_wire[0..len)
 * that starts at a frame header, followed on the device by the grouping of its
 * frames into messages, their out-of-place unmask and the UTF-8 check of the
 * reassembled TEXT messages. dev_wire is not modified; dev_frames and
 * *dev_result are what fws_gpu_decode_stream reports for the same bytes (the
 * first min(n_frames, cap) frames are grouped). Asynchronous on `stream`, no
 * host synchronisation, no device-to-host copy, and no allocation once
 * fws_gpu_ctx_reserve has sized the context. dev_wire and dev_dst are 16-B
 * aligned; dev_ctl may have any alignment.
 *   dev_dst   the unmasked payloads of the data frames (opcodes 0, 1, 2) in
 *             wire order: every message is one contiguous run, messages are
 *             packed back to back, the bytes present of an unfinished last
 *             message come last. If they exceed dst_cap nothing is written to
 *             dev_dst (FWS_ERR_CAPACITY; data_bytes is still reported, and no
 *             message gets a utf8_ok verdict).
 *   dev_ctl   the unmasked payloads of the complete control frames (opcodes 8,
 *             9, 10) packed in wire order (the ctl_out / ctl_off convention of
 *             fws_rx_session_feed); the same rule against ctl_cap.
 *   dev_msgs  entries [0, min(n_msgs, msg_cap)).
 * A truncated last payload contributes the bytes present and completes
 * nothing: a message whose FIN frame is truncated stays open, a truncated
 * control frame is neither listed nor copied. An unfinished message never gets
 * a utf8_ok verdict; the caller resubmits from resume_off.
 * status is the earliest problem in wire order:
 *   1. a sequencing error at frame e (err_frame = e): FWS_ERR_SEQUENCE for a
 *      continuation with no message open or a TEXT / BIN frame while one is
 *      open, FWS_ERR_CONTROL_FRAME for a control frame with FIN = 0 or a
 *      payload over 125 B. Frames e and later are neither gathered nor listed;
 *      the entries and bytes before e are delivered (as OnRecvData delivers
 *      what precedes an error) and the open-message fields describe the state
 *      just before e;
 *   2. else the parse's own status from *dev_result;
 *   3. else FWS_ERR_CAPACITY when n_frames > cap, n_msgs > msg_cap or a byte
 *      capacity was exceeded;
 *   4. else 0.
 * Every call starts from "no message open"; a connection whose bytes arrive in
 * reads uses fws_gpu_decode_messages_carry below, which carries the open
 * message and its UTF-8 state from call to call.
 * A CLOSE reason is validated where the CLOSE is answered
 * (fws_gpu_reply_messages_strict). Out of scope: client-side streams, the C++
 * adapter and the FLoop hook. */
int fws_gpu_decode_messages(fws_gpu_ctx *ctx, const void *dev_wire, uint64_t len,
                            fws_frame_info *dev_frames, uint32_t cap,
                            fws_msg_info *dev_msgs, uint32_t msg_cap,
                            void *dev_dst, uint64_t dst_cap,
                            void *dev_ctl, uint64_t ctl_cap,
                            fws_decode_result *dev_result, fws_msg_result *dev_msg_result,
                            void *stream);

/* ---- the same for a connection read by read --------------------------------
 * A connection delivers its bytes in reads; OnRecvData hands out a message's
 * parts as they arrive and carries a few words of state between reads
 * (w_socket.h:223-245, 713-747). fws_msg_carry is that state for
 * fws_gpu_decode_messages_carry, in device memory: the call's kernels read it
 * and rewrite it, so two calls queued on one stream chain through it without
 * the host. */
#define FWS_MSG_CONTINUED 1u     /* fws_msg_info.flags: the message began in an earlier call */

typedef struct fws_msg_carry {   /* device memory; all zero = a new connection */
    uint32_t open_opcode;        /* 0: no message open; 1 TEXT / 2 BIN */
    uint32_t open_frames;        /* data frames of the open message delivered so far (all calls) */
    uint64_t open_bytes;         /* its bytes delivered so far (all calls) */
    uint32_t utf8_tail;          /* open TEXT message: its last 3 delivered bytes, placed as the
                                    "previous dword" of the UTF-8 check (bits 31:24 the last byte,
                                    bits 7:0 zero; zeros where fewer than 3 exist) */
    uint32_t utf8_bad;           /* 1: the open TEXT message is already malformed (RFC 6455 §8.1
                                    allows failing early) */
    uint32_t prev_open_opcode;   /* open_opcode / open_frames / open_bytes as the last call found them: */
    uint32_t prev_open_frames;   /*   what a FWS_MSG_CONTINUED entry's len / n_data_frames add to */
    uint64_t prev_open_bytes;
    uint64_t wire_bytes;         /* running sum of resume_off over the calls */
    uint64_t n_msgs;             /* running count of entries delivered */
    uint64_t reserved;           /* 0 */
} fws_msg_carry;            /* 64 bytes */

/* fws_gpu_decode_messages for one read of a connection: dev_wire[0..len) is
 * the bytes from the previous call's resume_off on (what was left, then the
 * new read), starting at a frame header. *dev_carry is the connection's state
 * (NULL: FWS_ERR_INVALID). Stream-ordered like everything else here: no host
 * synchronisation, no device-to-host copy, no allocation after
 * fws_gpu_ctx_reserve. What is not listed is fws_gpu_decode_messages' contract
 * unchanged (the parse, dev_frames / *dev_result, the control frames' packing,
 * the status order, the alignment rules, dev_wire never written).
 *   initial state  the planner starts from the carry. With a message open a
 *             leading TEXT / BIN frame is FWS_ERR_SEQUENCE at that frame and a
 *             leading continuation is legal; with none open the other way round.
 *   whole frames   a truncated last frame, data or control, contributes
 *             nothing: it is not gathered, counted or sequence-checked, and
 *             resume_off is its hdr_off. Otherwise resume_off is the end of the
 *             last frame processed, or the failing header on a sequencing error.
 *             It never goes back to a message's first header. A frame must fit
 *             in the buffer the caller resubmits.
 *   parts     dev_dst holds this call's data bytes in wire order. A message
 *             completed here that began in an earlier call gets one entry with
 *             flags = FWS_MSG_CONTINUED whose off (always 0) / len /
 *             n_data_frames describe this call's part and whose first_frame is
 *             its first data frame of this call; the message's totals are
 *             prev_open_bytes + len and prev_open_frames + n_data_frames. The
 *             present bytes of a message still open at the end are a part too
 *             (open_off / open_len) and are never resubmitted. open_opcode != 0
 *             is the "open" test; open_first_frame is the message's first data
 *             frame in this call, 0xFFFFFFFF if it has none here.
 *   UTF-8     a TEXT entry's utf8_ok is the verdict on the whole message,
 *             earlier parts included: the call's first region takes utf8_tail
 *             as its left context and utf8_bad is sticky. The open TEXT part at
 *             the end is checked as a prefix (a sequence cut by its end is no
 *             error yet). An invalid byte (C0, C1, F5..FF) is flagged at the byte
 *             after it, so as a part's last byte it sets utf8_bad one call
 *             later; the final verdict is exact.
 *   errors    on a sequencing error at frame e the carry, like the open-message
 *             fields, describes the state just before e.
 *   capacity  n_frames > cap: FWS_ERR_CAPACITY, but the first cap frames are
 *             processed and the carry and resume_off are valid -- the caller
 *             continues from resume_off. data_bytes > dst_cap, ctl_bytes >
 *             ctl_cap or n_msgs > msg_cap: nothing is written to dev_dst or
 *             dev_ctl, *dev_carry is left exactly as found and resume_off = 0
 *             (the counts are still reported): the caller retries the same
 *             bytes with larger buffers.
 * Out of scope: resuming inside a frame's payload, client-side streams, the C++
 * adapter and the FLoop hook. */
int fws_gpu_decode_messages_carry(fws_gpu_ctx *ctx, const void *dev_wire, uint64_t len,
                                  fws_frame_info *dev_frames, uint32_t cap,
                                  fws_msg_info *dev_msgs, uint32_t msg_cap,
                                  void *dev_dst, uint64_t dst_cap,
                                  void *dev_ctl, uint64_t ctl_cap,
                                  fws_decode_result *dev_result, fws_msg_result *dev_msg_result,
                                  fws_msg_carry *dev_carry, void *stream);

/* ---- the same for the reads of many connections in one launch --------------
 * A server's loop step brings reads of a few KiB from many connections;
 * fws_gpu_decode_messages_carry is a sequence of launches per connection.
 * fws_gpu_decode_messages_multi decodes n reads in one launch, one workgroup
 * per read, the read staged in on-chip memory. Each read is described by a
 * fws_msg_read in device memory: where its bytes, its output regions and its
 * slices of the frame and entry arrays lie, and which carry is its
 * connection's. */
#define FWS_MSG_MULTI_MAX_READ   (128u << 10)   /* bytes of one read */
#define FWS_MSG_MULTI_MAX_FRAMES 256u           /* headers in one read */

typedef struct fws_msg_read {       /* device memory, one per read */
    uint64_t wire_off;              /* the read's bytes in dev_wire, 16-B aligned */
    uint64_t dst_off;               /* its region of dev_dst, 16-B aligned */
    uint64_t ctl_off;               /* its region of dev_ctl, any alignment */
    uint32_t len;                   /* bytes of wire (0 allowed) */
    uint32_t conn;                  /* index into dev_carries, < n_conns; distinct within a call */
    uint32_t dst_cap, ctl_cap;      /* bytes */
    uint32_t frame_base, frame_cap; /* its slice of dev_frames */
    uint32_t msg_base, msg_cap;     /* its slice of dev_msgs */
    uint64_t reserved;              /* 0 */
} fws_msg_read;                     /* 64 bytes */

/* For read r, everything the call writes -- its frame slice, its entries, its
 * regions of dev_dst and dev_ctl, dev_results[r], dev_msg_results[r] and
 * dev_carries[conn] -- is byte for byte what fws_gpu_decode_messages_carry
 * writes for the same bytes, the same four capacities and the same carry, with
 * every offset and index relative to the read (hdr_off, fws_msg_info.off,
 * first_frame, resume_off, open_off ...). One exception:
 * fws_decode_result.n_survivors, a diagnostic, is n_frames. The contract of
 * fws_gpu_decode_messages_carry above holds per read unchanged.
 *   isolation   an error on one connection -- protocol, sequencing, capacity --
 *             changes nothing for any other. The call returns 0 whenever the
 *             launch was made; per-read outcomes are dev_msg_results[r].status.
 *   declined    a read with len > max_len, len > FWS_MSG_MULTI_MAX_READ or more
 *             than FWS_MSG_MULTI_MAX_FRAMES headers: both results get status =
 *             FWS_ERR_DECLINED and every other field zero, but err_frame and
 *             open_first_frame = 0xFFFFFFFF; nothing else is written for that
 *             read and its carry is untouched. The caller runs
 *             fws_gpu_decode_messages_carry on the same bytes with the same
 *             carry and the connection continues exactly.
 *   descriptors a misaligned wire_off or dst_off, or conn >= n_conns: both
 *             results get FWS_ERR_INVALID in the same way. Two reads of one call
 *             that name the same conn are a contract violation: the result is
 *             undefined for that connection only.
 *   max_len   the caller's upper bound on len (it built the descriptors),
 *             between 1 and FWS_MSG_MULTI_MAX_READ. It selects the kernel form:
 *             up to 16 KiB a small workgroup, several to a compute unit; above,
 *             one workgroup to a compute unit.
 *   ordering  stream-ordered: no host synchronisation, no device-to-host copy;
 *             no workspace, so nothing is allocated, with or without
 *             fws_gpu_ctx_reserve. Two calls queued on one stream chain through
 *             the carries; a captured call needs no reset node.
 * n == 0 returns 0 without a launch. Otherwise ctx and every pointer must be
 * non-null, dev_wire and dev_dst 16-B aligned and max_len in range, or the call
 * returns FWS_ERR_INVALID before any device call. Out of scope as above. */
int fws_gpu_decode_messages_multi(fws_gpu_ctx *ctx, const void *dev_wire,
                                  const fws_msg_read *dev_reads, uint32_t n, uint32_t max_len,
                                  fws_frame_info *dev_frames, fws_msg_info *dev_msgs,
                                  void *dev_dst, void *dev_ctl,
                                  fws_decode_result *dev_results, fws_msg_result *dev_msg_results,
                                  fws_msg_carry *dev_carries, uint32_t n_conns, void *stream);

/* ---- the same, resuming inside a frame: any cut, frames of any size ---------
 * The calls above take whole frames, so a frame has to fit in the bytes of one
 * call. OnRecvData hands out a frame's payload as it arrives (unread_pl_len_
 * and the rotated key, w_socket.h:223-245, 756-759) and accepts frames up to
 * 2^32 B (w_socket.h:493-498). fws_gpu_decode_messages_flow is the one-launch,
 * many-connections call with a state per connection that also holds a data
 * frame in progress: a read may begin inside a data frame's payload and end
 * inside one. */
typedef struct fws_msg_flow {      /* device memory; all zero = a new connection */
    fws_msg_carry msg;             /* exactly what fws_gpu_decode_messages_carry keeps */
    uint64_t frame_unread;         /* payload bytes of the data frame in progress still to come; 0: between frames */
    uint64_t frame_len;            /* that frame's payload_len (0 when frame_unread == 0) */
    uint32_t frame_key;            /* its key rotated to the next byte to come: rotr(key, 8 * (delivered & 3)),
                                      the reference's RotateR (w_socket.h:756-759), fws_rx_state.mask_key */
    uint8_t  frame_fin;            /* its FIN bit */
    uint8_t  pad[3];               /* 0 */
    uint64_t reserved;             /* 0 */
} fws_msg_flow;                    /* 96 bytes */

/* Arguments, alignment rules, the argument checks before any device call,
 * n == 0, the fws_msg_read descriptor, the kernel form chosen by max_len,
 * isolation, stream ordering and the absence of a workspace are those of
 * fws_gpu_decode_messages_multi; offsets and indices are relative to the read.
 * With frame_unread == 0 and a read of whole frames every byte written equals
 * that call's (dev_flows[conn].msg its carry, the frame fields zero). What
 * differs:
 *   input     a read's bytes are what was left from the previous call's
 *             resume_off, then the new bytes. With frame_unread > 0 the first
 *             lead = min(frame_unread, len) bytes are payload of the frame in
 *             progress and the header chain starts at lead; else at 0.
 *   data frames are taken as they arrive: a data frame with a complete header is
 *             sequence-checked against the open state, then its present bytes
 *             (zero allowed) are gathered and counted even when the payload runs
 *             past the end. The state then records frame_unread / frame_len /
 *             frame_key / frame_fin, the message stays open, resume_off = len;
 *             the present bytes belong to the open part (open_off / open_len).
 *             A frame counts in n_data_frames, open_frames and the entries in
 *             the call that holds its header; the lead counts bytes only.
 *   the lead  goes to dev_dst from offset 0, unmasked with frame_key from phase
 *             0. If it ends the frame (frame_unread <= len) and frame_fin is
 *             set, the message completes there with a FWS_MSG_CONTINUED entry:
 *             off = 0, len and n_data_frames this call's part, first_frame /
 *             last_frame the message's first and last data frames whose header
 *             is in this call, 0xFFFFFFFF if none. With frame_fin = 0 the chain
 *             goes on with the message open. If it does not end the frame the
 *             read is all payload: n_frames = 0, frame_unread shrinks by len,
 *             frame_key is rotated by len & 3.
 *   control frames stay whole: one whose payload is cut is not processed and
 *             resume_off is its header; an incomplete trailing header is left
 *             as well. A caller's pending bytes are fewer than 14 + 125.
 *   dev_frames / fws_decode_result describe the headers in this read: hdr_off
 *             relative to the read start (lead included), FWS_FRAME_TRUNCATED on
 *             a cut last frame, carry_unread the bytes still to come of whatever
 *             frame is in progress at the end, consumed = len unless a partial
 *             header remains or an error or the header limit stopped the walk.
 *   UTF-8     as fws_gpu_decode_messages_carry: each call's part starts at
 *             dev_dst + 0, utf8_tail is its left context, utf8_bad is sticky;
 *             the final verdict is exact wherever the cuts fell, inside a frame
 *             and inside a sequence included.
 *   headers   no read is declined for its header count. At header number
 *             FWS_MSG_MULTI_MAX_FRAMES + 1 the walk stops as at an exceeded
 *             frame_cap: the first min(frame_cap, FWS_MSG_MULTI_MAX_FRAMES)
 *             frames are processed, n_frames counts the headers parsed (at most
 *             FWS_MSG_MULTI_MAX_FRAMES + 1), consumed is that header's offset,
 *             status = FWS_ERR_CAPACITY unless there is an earlier problem, the
 *             state and resume_off are valid and the caller continues from
 *             resume_off. FWS_ERR_DECLINED remains for len > max_len or len >
 *             FWS_MSG_MULTI_MAX_READ; FWS_ERR_INVALID per descriptor as above.
 *   errors    a sequencing or control-frame-form error at frame e gives the
 *             state just before e (frame_unread = 0: e is a header). A cut data
 *             frame that fails the sequence check is an error and is not taken.
 *   capacity  data_bytes > dst_cap, ctl_bytes > ctl_cap or n_msgs > msg_cap:
 *             nothing is written to dev_dst / dev_ctl, the whole 96-byte state
 *             is left exactly as found and resume_off = 0. A call never
 *             produces more data bytes than it was given: dst_cap >= len is
 *             always enough.
 * A read longer than FWS_MSG_MULTI_MAX_READ is cut anywhere into pieces whose
 * calls are queued on one stream; they chain through dev_flows without the
 * host. This is the server role: every frame must be masked. A client's
 * connections use fws_gpu_decode_messages_flow_client below. Out of scope: the
 * same for fws_gpu_decode_messages(_carry), the C++ adapter and the FLoop hook. */
int fws_gpu_decode_messages_flow(fws_gpu_ctx *ctx, const void *dev_wire,
                                 const fws_msg_read *dev_reads, uint32_t n, uint32_t max_len,
                                 fws_frame_info *dev_frames, fws_msg_info *dev_msgs,
                                 void *dev_dst, void *dev_ctl,
                                 fws_decode_result *dev_results, fws_msg_result *dev_msg_results,
                                 fws_msg_flow *dev_flows, uint32_t n_conns, void *stream);

/* ---- the same for a client's connections -------------------------------------
 * OnRecvData is templated on the role (WSClientSocket / WSServerSocket); what a
 * client receives are server frames: no MASK bit, no key, payload in the clear
 * (w_socket.h:518-521). fws_gpu_decode_messages_flow_client is
 * fws_gpu_decode_messages_flow in that role. The arguments, the argument checks
 * before any device call, n == 0, the fws_msg_read descriptors, the fws_msg_flow
 * state, the kernel form chosen by max_len, isolation, ordering, the header
 * limit, the capacity rules and every field written are that call's. What
 * differs, and nothing else:
 *   headers   are parsed in the client role. A header with the MASK bit set is
 *             FWS_ERR_MASKED at that header, reported exactly as the other parse
 *             errors are: fws_decode_result.status / err_off / consumed, and
 *             fws_msg_result.status by the status order, the frames before it
 *             delivered. A header is 2, 4 or 10 bytes: fws_frame_info.hdr_len is
 *             one of these and fws_frame_info.key is 0. FWS_ERR_NOT_MASKED never
 *             occurs.
 *   payload   data and control payload bytes are copied as they are (an unmask
 *             with key 0). The UTF-8 check, the entries, the open part,
 *             FWS_MSG_CONTINUED, the lead and frame_unread / frame_len /
 *             frame_fin are unchanged; frame_key is always 0.
 *   control frames stay whole as there; a caller's pending bytes are fewer than
 *             10 + 125.
 *   headers per read  a frame may be as short as 2 bytes, so a read of len bytes
 *             holds up to len / 2 headers (the server role: len / 6). The walk
 *             still stops at header FWS_MSG_MULTI_MAX_FRAMES + 1 and the caller
 *             continues from resume_off; a frame_cap of
 *             min(len / 2 + 1, FWS_MSG_MULTI_MAX_FRAMES) never limits a read.
 *   state     a connection's fws_msg_flow belongs to one role: it is written by
 *             this call only or by fws_gpu_decode_messages_flow only. Mixing the
 *             two on one state is a contract violation (the server role's
 *             frame_key would be dropped).
 * fws_gpu_reply_messages_multi_client / _strict_client answer what this call
 * delivered with masked frames. Out of scope: a client role for
 * fws_gpu_decode_messages, _carry, _multi, fws_gpu_decode_stream and
 * fws_rx_session; the C++ adapter and the FLoop hook. */
int fws_gpu_decode_messages_flow_client(fws_gpu_ctx *ctx, const void *dev_wire,
                                        const fws_msg_read *dev_reads, uint32_t n, uint32_t max_len,
                                        fws_frame_info *dev_frames, fws_msg_info *dev_msgs,
                                        void *dev_dst, void *dev_ctl,
                                        fws_decode_result *dev_results, fws_msg_result *dev_msg_results,
                                        fws_msg_flow *dev_flows, uint32_t n_conns, void *stream);

/* ---- batched stream decode: many independent streams ----------------------
 * fws_gpu_decode_stream over a list of independent streams (the buffers of
 * many connections, or successive batches of one: FLoop's loop hands each
 * socket's bytes to its own OnRecvData, floop.h:661-703), with decodes kept
 * in flight on two HIP streams so one job's latency-bound resolve overlaps
 * another's streaming kernels. Each job's frames, result,
 * UTF-8 flags and unmasked bytes equal fws_gpu_decode_stream on that job
 * alone. Jobs must not share memory. The work is ordered after everything
 * already on `stream`, and `stream` waits for all of it (synchronise `stream`
 * to read results). An engine is used from one host thread at a time; it owns
 * its workspaces, sized by max_frames / max_stream_bytes per job (a larger job
 * grows them after draining the engine). */
typedef struct fws_decode_job {
    void *dev_wire;                 /* 16-B aligned, as fws_gpu_decode_stream */
    uint64_t len;
    fws_frame_info *dev_frames;
    uint32_t cap;
    uint32_t reserved;              /* 0 */
    fws_decode_result *dev_result;
    uint8_t *dev_utf8_ok;           /* optional (NULL) */
} fws_decode_job;                   /* 48 bytes */

typedef struct fws_decode_engine fws_decode_engine;
int fws_decode_engine_create(int device, uint64_t max_frames, uint64_t max_stream_bytes, fws_decode_engine **out);
void fws_decode_engine_destroy(fws_decode_engine *e);
int fws_decode_engine_run(fws_decode_engine *e, const fws_decode_job *jobs, uint32_t n, void *stream);

/* Per-frame UTF-8 validation of already-unmasked payloads (Unicode Table
 * 3-7): ok[i] = 1 iff region i is well-formed UTF-8. */
int fws_gpu_validate_utf8(fws_gpu_ctx *ctx, const void *dev_base, const fws_frame_desc *dev_descs,
                          uint32_t n, uint8_t *dev_ok, void *stream);

/* ---- host-buffer RX session: OnRecvData over the GPU ----------------------
 * Mirrors WSocket::OnRecvData (w_socket.h:543-769) for one server
 * connection: reads are host buffers, decode runs on the device, and the
 * on_read() contract (opcode, part, is_frame_end, is_msg_end, is_control) is
 * reported as an event array whose order and values match the reference.
 * Control frames: PING -> a PONG event (the caller sends the reply), CLOSE ->
 * a CLOSE event with status code; their payload bytes are copied to ctl_out. */
typedef struct fws_rx_event {
    uint32_t kind;          /* 0 ON_READ, 1 PONG_TO_SEND, 2 CLOSE_RECEIVED */
    uint32_t opcode;        /* reported opcode (continuations report the first frame's, w_socket.h:626) */
    uint8_t is_ctl;
    uint8_t frame_end;
    uint8_t msg_end;
    uint8_t fin;
    uint32_t code;          /* CLOSE status code (1005 if absent) */
    uint64_t size;          /* bytes in this part */
    uint64_t data_off;      /* ON_READ data part: offset of the part in the read buffer */
    uint64_t ctl_off;       /* control payload copy offset in ctl_out */
    uint64_t capacity;      /* IOBuffer capacity of the view, relative to the read start */
} fws_rx_event;             /* 48 bytes */

/* Carried RX state of a session (w_socket.h:223-245), for inspection. */
typedef struct fws_rx_state {
    int32_t recv_status;    /* 0 WAIT_FRAME_HEAD, 1 WAIT_FRAME_PAYLOAD */
    uint32_t mask_key;      /* last_rx_mask_key_, rotated for the next payload byte */
    uint64_t unread_pl_len;
    uint8_t last_rx_opcode;
    uint8_t last_rx_control_opcode;
    uint8_t last_rx_fin_flag;
    uint8_t is_rx_control_frame;
    uint32_t last_rx_hdr_part_len;
} fws_rx_state;             /* 24 bytes */

typedef struct fws_rx_session fws_rx_session;

int fws_rx_session_create(fws_gpu_ctx *ctx, int is_server, fws_rx_session **out);
void fws_rx_session_destroy(fws_rx_session *s);
/* Decode one read in place (buf is host memory, unmasked on return). Returns
 * 0 or the reference's negative ParseFrameHdr code. buf_capacity: the view's
 * capacity measured from buf (the last part's IOBuffer capacity). */
int fws_rx_session_feed(fws_rx_session *s, uint8_t *buf, uint64_t size, uint64_t buf_capacity,
                        fws_rx_event *events, uint64_t ev_cap, uint64_t *n_events,
                        uint8_t *ctl_out, uint64_t ctl_cap, uint64_t *ctl_used);
int fws_rx_session_state(const fws_rx_session *s, fws_rx_state *out);
/* fws_rx_session_feed with the session's own event and control-payload sinks
 * (grown as needed, no capacity error): *events / *ctl point into the session
 * and stay valid until its next feed. */
int fws_rx_session_feed_view(fws_rx_session *s, uint8_t *buf, uint64_t size, uint64_t buf_capacity,
                             const fws_rx_event **events, uint64_t *n_events, const uint8_t **ctl,
                             uint64_t *ctl_used);
/* The last feed's protocol error (0 if none) and the opcode of the frame it
 * stopped at, for the reference's error text ("Opcode %u is not valid",
 * w_socket.h:452) in the Close reason (ws_server_socket.h:178-181). */
int fws_rx_session_error(const fws_rx_session *s, uint32_t *opcode);

/* ---- many connections, one round trip -----------------
 * FLoop::OneStep (floop.h:661-703) drains every readable socket in one loop
 * iteration and runs each read through its socket's OnRecvData. fws_rx_mux
 * keeps one RX state per connection (the fws_rx_session of each) and decodes
 * the reads of many connections -- each with its own carried state: staged
 * header bytes, unread payload of the frame in progress, rotated key -- with
 * one pinned staging pass, one H2D copy, one launch (one workgroup per read)
 * and one D2H copy, then replays each connection's OnRecvData bookkeeping.
 * Per read the results equal fws_rx_session_feed on that connection alone.
 * A read over 256 KiB, or whose header stream needs the parallel decode (over
 * 128 KiB or 256 headers), goes through that connection's session path. */
typedef struct fws_rx_mux fws_rx_mux;
typedef struct fws_rx_read {
    uint32_t conn;          /* connection slot, < n_conns; at most one read per slot per call */
    uint32_t flags;         /* 0 */
    uint8_t *buf;           /* host memory, unmasked in place */
    uint64_t size;
    uint64_t capacity;      /* the view's capacity from buf (fws_rx_session_feed) */
} fws_rx_read;
typedef struct fws_rx_read_result {
    int32_t ret;            /* fws_rx_session_feed's return for this read */
    uint32_t pad;
    const fws_rx_event *events;   /* the connection's events, valid until its next feed */
    uint64_t n_events;
    const uint8_t *ctl;           /* control payloads the events point into */
    uint64_t ctl_used;
} fws_rx_read_result;
int fws_rx_mux_create(fws_gpu_ctx *ctx, uint32_t n_conns, fws_rx_mux **out);
void fws_rx_mux_destroy(fws_rx_mux *m);
/* slot `conn` starts a new connection (the reference's initial RX state) */
int fws_rx_mux_reset(fws_rx_mux *m, uint32_t conn);
int fws_rx_mux_state(const fws_rx_mux *m, uint32_t conn, fws_rx_state *out);
int fws_rx_mux_error(const fws_rx_mux *m, uint32_t conn, uint32_t *opcode);
/* Decode n reads (distinct connections). Returns 0 (per-read codes in
 * results[i].ret) or FWS_ERR_INVALID / a HIP error for the call itself. */
int fws_rx_mux_feed(fws_rx_mux *m, const fws_rx_read *reads, uint32_t n, fws_rx_read_result *results);
/* fws_rx_mux_feed in two halves, so the host can go on (read more sockets,
 * dispatch an earlier batch's events) while the GPU decodes: submit stages and
 * starts the batch and returns; complete waits for it and fills results[0, n)
 * exactly as feed would. One batch at a time: submit again only after
 * complete. Until complete returns the reads' buffers belong to the mux
 * (unmasked in place), and the connections' state is the state before the
 * batch. Other GPU calls of the context may be made in between (a request of
 * the context's persistent receive decode waits for the batch first). */
int fws_rx_mux_submit(fws_rx_mux *m, const fws_rx_read *reads, uint32_t n);
int fws_rx_mux_complete(fws_rx_mux *m, fws_rx_read_result *results);
/* Non-blocking: 1 when fws_rx_mux_complete would not wait (the submitted
 * batch has decoded, or none is in flight), 0 while it decodes, < 0 on a HIP
 * error. The batched hook's deferred completion polls it (gpu_floop.hpp). */
int fws_rx_mux_ready(fws_rx_mux *m);

/* ---- send path: batch frame builder -------------------
 * The bytes WSocket::SendFrame (w_socket.h:832-944) writes for one frame:
 * b0 = FIN << 7 | opcode, b1 = MASK << 7 | len7, the BE 16 / 64-bit length,
 * for a client frame the key (native LE u32 of the wire bytes) and the payload
 * XORed with it from phase 0 (w_socket.h:858-866). The reference draws the key
 * from SemiSecureRand32 (w_socket.h:860); here the caller supplies it. */
typedef struct fws_tx_desc {
    uint64_t src_off;       /* payload bytes at dev_src + src_off */
    uint64_t len;           /* payload length */
    uint32_t key;           /* mask key (masked frames) */
    uint8_t opcode;         /* wire opcode: 0 continuation, 1 TEXT, 2 BIN, 8 CLOSE, 9 PING, 10 PONG */
    uint8_t fin;
    uint8_t masked;         /* 1: client frame (MASK bit + key + masked payload); 0: server frame */
    uint8_t pad;
} fws_tx_desc;              /* 24 bytes */

/* Opcode and FIN of a connection's next frame by SendFrame's rule
 * (w_socket.h:845-848, 903-913): a data frame that continues an unfinished
 * message is a continuation; control frames neither use nor change the state.
 * frame_type: WSTxFrameType (1 TEXT, 2 BIN, 8 CLOSE, 9 PING, 10 PONG). Host code. */
void fws_tx_next(uint32_t frame_type, int last_frame_if_possible, uint8_t *last_msg_not_fin, uint8_t *opcode,
                 uint8_t *fin);

/* dev_out (16-B aligned) = the frames of dev_descs[0..n) back to back;
 * *dev_out_len (device u64) = their total size, or ~0 if it exceeds out_cap.
 * The default form (plan + encode: k_out_plan, k_tx_encode_w5) writes nothing
 * when the total exceeds out_cap. The opt-in one-launch tuning form (k_tx_one,
 * fws_internal_set_tx_one; measured slower) never writes a
 * byte at or past out_cap, but writes the frames that fit below it. */
int fws_gpu_encode_frames(fws_gpu_ctx *ctx, void *dev_out, uint64_t out_cap, const void *dev_src,
                          const fws_tx_desc *dev_descs, uint32_t n, uint64_t *dev_out_len, void *stream);

/* ---- the sends of many connections encoded in one launch --------------------
 * The TX counterpart of fws_gpu_decode_messages_multi: n sends, one workgroup
 * per send, each into its own region of dev_out. A send is one payload; the
 * device cuts it into frames of max_frame payload bytes and takes opcode and FIN
 * from the connection's state in device memory (SendFrame's rule, fws_tx_next),
 * which it reads and rewrites, so replies need no host round trip and no
 * per-frame descriptor. */
#define FWS_TX_MULTI_MAX_SEND   (128u << 10)   /* payload bytes of one send */
#define FWS_TX_MULTI_MAX_FRAMES 256u           /* frames one send may be cut into */
/* key of a masked send's fragment j (j = 0: the send's key) */
#define FWS_TX_FRAG_KEY(key, j) ((uint32_t)((key) + (uint32_t)(j) * 0x9E3779B9u))

typedef struct fws_tx_conn {        /* device memory; all zero = a new connection */
    uint32_t last_msg_not_fin;      /* SendFrame's last_msg_not_fin_ (fws_tx_next) */
    uint32_t reserved0;             /* 0 */
    uint64_t frames;                /* running count of frames written */
    uint64_t wire_bytes;            /* running sum of out_len */
    uint64_t reserved;              /* 0 */
} fws_tx_conn;                      /* 32 bytes */

typedef struct fws_tx_send {        /* device memory, one per send */
    uint64_t src_off;               /* payload at dev_src + src_off, any alignment */
    uint64_t out_off;               /* its region of dev_out, 16-B aligned */
    uint32_t len;                   /* payload bytes (0 allowed) */
    uint32_t out_cap;               /* bytes of the region */
    uint32_t conn;                  /* index into dev_conns, < n_conns; distinct within a call */
    uint32_t max_frame;             /* data sends: payload bytes per frame; 0 = one frame */
    uint32_t key;                   /* masked sends */
    uint8_t  frame_type;            /* WSTxFrameType: 1 TEXT, 2 BIN, 8 CLOSE, 9 PING, 10 PONG */
    uint8_t  last;                  /* last_frame_if_possible of the send's last frame */
    uint8_t  masked;                /* 1 client frames, 0 server frames */
    uint8_t  pad;                   /* 0 */
    uint32_t frame_base, frame_cap; /* its slice of dev_frames (frame_cap 0: no records) */
    uint64_t reserved[2];           /* 0 */
} fws_tx_send;                      /* 64 bytes */

typedef struct fws_tx_result {
    int32_t  status;
    uint32_t n_frames;              /* frames of the send, also past frame_cap */
    uint64_t out_len;               /* bytes written; on FWS_ERR_CAPACITY the bytes needed */
    uint32_t last_msg_not_fin;      /* the connection's state after the send */
    uint32_t pad;
    uint64_t reserved;
} fws_tx_result;                    /* 32 bytes */

/* Per send s (offsets relative to the send's region, dev_out + out_off):
 *   frames    a control send (frame_type & 8) is one frame, max_frame ignored. A
 *             data send with max_frame == 0 or len <= max_frame is one frame
 *             (len == 0: one empty frame). Otherwise k = ceil(len / max_frame)
 *             frames, the first k - 1 of max_frame payload bytes, the last of
 *             the rest. Frame j's opcode and FIN are what
 *             fws_tx_next(frame_type, j == k - 1 ? last : 0, &state, ...) gives
 *             for frames 0 .. k - 1 in order from dev_conns[conn].last_msg_not_fin:
 *             exactly k SendFrame calls. A control send neither uses nor changes
 *             the state; its FIN is `last`.
 *   bytes     the frames back to back from the region's start, each what
 *             fws_gpu_encode_frames writes for the same payload slice, opcode,
 *             FIN, mask bit and key; frame j of a masked send uses
 *             FWS_TX_FRAG_KEY(key, j), XORed from phase 0. No byte outside
 *             [out_off, out_off + out_len) is written, inside out_cap or not (a
 *             tail of out_len % 16 bytes is stored partially). Regions of
 *             different sends must not overlap.
 *   state     on success dev_conns[conn] gets the new last_msg_not_fin,
 *             frames += n_frames, wire_bytes += out_len; the result echoes the new
 *             last_msg_not_fin.
 *   records   dev_frames[frame_base + j], j < min(n_frames, frame_cap): hdr_off
 *             (relative to the region), payload_len, key (0 when unmasked), the
 *             wire opcode, fin, hdr_len, flags = 0 -- for a masked send the
 *             records fws_gpu_decode_messages_flow reports for the same bytes.
 *             frame_cap < n_frames is not an error. dev_frames may be NULL when
 *             every frame_cap is 0: the kernel then never dereferences it.
 *   refusals  per send; the call still returns 0 and other sends are untouched.
 *             Nothing is written to the region, the records or the state, and
 *             the result's other fields are zero except where stated. Tested in
 *             this order:
 *               FWS_ERR_INVALID        out_off not 16-B aligned, conn >= n_conns,
 *                                      frame_type not 1, 2, 8, 9 or 10
 *               FWS_ERR_CONTROL_FRAME  a control send with len > 125
 *               FWS_ERR_DECLINED       len > max_len, len > FWS_TX_MULTI_MAX_SEND
 *                                      or more than FWS_TX_MULTI_MAX_FRAMES frames:
 *                                      split the send, or use fws_gpu_encode_frames
 *               FWS_ERR_CAPACITY       the bytes needed exceed out_cap; out_len =
 *                                      the bytes needed, n_frames is set (the
 *                                      count is closed-form: known before the
 *                                      first store)
 *             Two sends of one call that name the same conn are a contract
 *             violation: the result is undefined for that connection only.
 *   streaming a message over FWS_TX_MULTI_MAX_SEND goes as sends of at most that
 *             size, each a multiple of max_frame, `last` on the final one only, in
 *             successive calls on one stream: the state makes the pieces' frames
 *             continuations. Each piece of a masked message restarts its keys at
 *             its own `key` (the reference draws a fresh key per frame,
 *             w_socket.h:860, so any key is as good).
 *   max_len   the caller's upper bound on len, between 1 and
 *             FWS_TX_MULTI_MAX_SEND. It selects the kernel form: up to 16 KiB a
 *             workgroup of 256 threads, above one of 1024.
 *   ordering  stream-ordered: no host synchronisation, no device-to-host copy, no
 *             allocation, no workspace. Two calls queued on one stream chain
 *             through dev_conns; a captured call needs no reset node.
 * n == 0 returns 0 without a launch. Otherwise ctx and every pointer but
 * dev_frames must be non-null, dev_out 16-B aligned and max_len in range, or the
 * call returns FWS_ERR_INVALID before any device call. Out of scope: two sends
 * of one connection in one call. */
int fws_gpu_encode_messages_multi(fws_gpu_ctx *ctx, void *dev_out, const void *dev_src,
                                  const fws_tx_send *dev_sends, uint32_t n, uint32_t max_len,
                                  fws_frame_info *dev_frames, fws_tx_result *dev_results,
                                  fws_tx_conn *dev_conns, uint32_t n_conns, void *stream);

/* ---- replies built on the device ----------------------------------------------
 * The link between the two halves above. OnRecvData answers a completed PING
 * with a PONG carrying the same payload (w_socket.h:661-666) and a completed
 * CLOSE with a CLOSE carrying the same payload unless one was sent already
 * (w_socket.h:667-710); an echo server sends every message back.
 * fws_gpu_reply_messages_multi reads what fws_gpu_decode_messages_flow or
 * fws_gpu_decode_messages_multi wrote for dev_reads[0..n) and writes each
 * read's reply frames into its own region of dev_out, one workgroup per read:
 * decode -> reply runs on one stream with no host in between. */
#define FWS_REPLY_CONTROL 1u   /* PING -> PONG, CLOSE -> CLOSE (w_socket.h:661-710) */
#define FWS_REPLY_ECHO    2u   /* every data part goes back as one frame */

typedef struct fws_reply_state {   /* device memory, one per connection; all zero = new */
    uint32_t close_sent;   /* 1: this connection's CLOSE has been written (or the host sent one and
                              set it, the reference's HasSentClose): the call writes nothing more */
    uint32_t close_code;   /* status code of the CLOSE received: big-endian u16 of its first two
                              payload bytes, 1005 when it has fewer than two (w_socket.h:668-673); 0 before */
    uint32_t fail_code;    /* fws_gpu_reply_messages_strict: the status code this side sent when it failed
                              the connection (1002, 1007 or 1009); 0 otherwise, and always 0 from
                              fws_gpu_reply_messages_multi */
    uint32_t reserved;     /* 0 */
} fws_reply_state;         /* 16 bytes */

typedef struct fws_reply_region {  /* device memory, one per read */
    uint64_t out_off;               /* the read's region of dev_out, 16-B aligned */
    uint32_t out_cap;
    uint32_t frame_base, frame_cap; /* its slice of dev_frames (frame_cap 0: no records) */
    uint32_t reserved0;
    uint64_t reserved;
} fws_reply_region;                 /* 32 bytes */

/* dev_reads, n, max_len, dev_msgs, dev_dst, dev_ctl and dev_msg_results are the
 * decode call's own arguments; the call only reads them. dev_conns is the array
 * an application hands to fws_gpu_encode_messages_multi for its own sends, so
 * the two calls sequence one connection's frames through one state. Per read r
 * (conn = dev_reads[r].conn, offsets relative to the region dev_out + out_off):
 *   no frames  status 0, n_frames 0, out_len 0, neither state changed, when the
 *             read's fws_msg_result.status is FWS_ERR_DECLINED or
 *             FWS_ERR_INVALID; when its decode delivered nothing (n_msgs >
 *             msg_cap, data_bytes > dst_cap or ctl_bytes > ctl_cap, the
 *             capacities taken from the read's descriptor); or when
 *             dev_states[conn].close_sent is set.
 *   frames    every other status (0, a protocol or sequencing error, a frame-count
 *             FWS_ERR_CAPACITY) leaves a valid prefix: n_msgs entries, then the
 *             open part open_off / open_len. In this order:
 *             1. per entry: opcode 9 with FWS_REPLY_CONTROL one PONG frame, FIN =
 *                1, payload dev_ctl[ctl_off + off, +len); opcode 10 nothing;
 *                opcode 8 with FWS_REPLY_CONTROL one CLOSE frame with the same
 *                payload whatever its length (w_socket.h:693), close_sent = 1
 *                and close_code set, every later item of the read dropped;
 *                opcode 1 or 2 with FWS_REPLY_ECHO one data frame, payload
 *                dev_dst[dst_off + off, +len) (len 0: an empty frame),
 *                frame_type the entry's opcode, last = 1;
 *             2. the open part, with FWS_REPLY_ECHO, when open_opcode != 0 and
 *                open_len > 0: one data frame of [open_off, +open_len), frame_type
 *                open_opcode, last = 0.
 *             Opcode and FIN of the data frames are what fws_tx_next(frame_type,
 *             last, &state, ...) gives, applied in that order from
 *             dev_conns[conn].last_msg_not_fin: a part whose earlier parts were
 *             echoed is a continuation by itself; an open part of 0 bytes gives
 *             no frame, so the frame that completes it carries the opcode.
 *             Control frames neither use nor change the state.
 *   bytes     server frames (no MASK bit, no key) back to back from the region's
 *             start, each what fws_gpu_encode_frames writes for that payload,
 *             opcode and FIN. No byte outside [out_off, out_off + out_len) is
 *             written. Sources may have any alignment. Regions must not overlap.
 *   state     on success dev_conns[conn] gets the new last_msg_not_fin, frames +=
 *             n_frames, wire_bytes += out_len; dev_states[conn] as above. The
 *             result echoes the connection's last_msg_not_fin after the call.
 *   records   dev_frames[frame_base + j], j < min(n_frames, frame_cap), as
 *             fws_gpu_encode_messages_multi writes them: hdr_off relative to the
 *             region, key 0. dev_frames may be NULL when every frame_cap is 0.
 *   refusals  per read; the call still returns 0, nothing is written for that
 *             read but its result (other fields zero except where stated) and
 *             both states are untouched. Tested in this order, around the "no
 *             frames" tests:
 *               FWS_ERR_INVALID   out_off not 16-B aligned or conn >= n_conns
 *                                 (before anything else)
 *               (no frames: the decode's status, an undelivered decode)
 *               FWS_ERR_INVALID   n_msgs > FWS_MSG_MULTI_MAX_FRAMES + 1 with
 *                                 n_msgs <= msg_cap: not a decode output
 *               (no frames: close_sent)
 *               FWS_ERR_INVALID   an entry no decode writes: a PING or CLOSE over
 *                                 125 bytes, a data part over
 *                                 FWS_MSG_MULTI_MAX_READ, an open_opcode not 1 or 2
 *               FWS_ERR_CAPACITY  the bytes needed exceed out_cap; out_len = the
 *                                 bytes needed, n_frames is set. The inputs are
 *                                 intact: the caller may call again with a
 *                                 larger region.
 *             Two reads of one call that name the same conn are a contract
 *             violation: the result is undefined for that connection only.
 *   max_len   the decode call's value; it selects the workgroup form as there.
 *   ordering  stream-ordered: no host synchronisation, no copy, no allocation, no
 *             workspace. Calls queued on one stream chain through dev_conns and
 *             dev_states; a captured call needs no reset node.
 * n == 0 returns 0 and looks at nothing. Otherwise ctx and every pointer but
 * dev_frames must be non-null, dev_out 16-B aligned, max_len between 1 and
 * FWS_MSG_MULTI_MAX_READ and flags within the two bits defined, or the call
 * returns FWS_ERR_INVALID before any device call. A client's replies, which must
 * be masked, are fws_gpu_reply_messages_multi_client's below. Out of scope:
 * cutting a part into several frames; the C++ adapter and the FLoop hook. This
 * call answers whatever the
 * decode delivered -- a TEXT entry with utf8_ok == 0 is echoed like any other, a
 * decode that ended in a protocol error gets the replies to its valid prefix;
 * fws_gpu_reply_messages_strict below fails such a connection instead. */
int fws_gpu_reply_messages_multi(fws_gpu_ctx *ctx,
                                 const fws_msg_read *dev_reads, uint32_t n, uint32_t max_len,
                                 const fws_msg_info *dev_msgs, const void *dev_dst, const void *dev_ctl,
                                 const fws_msg_result *dev_msg_results,
                                 const fws_reply_region *dev_regions, void *dev_out,
                                 fws_frame_info *dev_frames, fws_tx_result *dev_results,
                                 fws_tx_conn *dev_conns, fws_reply_state *dev_states, uint32_t n_conns,
                                 uint32_t flags, void *stream);

/* ---- the same for a server that fails connections on the device ---------------
 * RFC 6455 §7.1.7 ("Fail the WebSocket Connection"), §5.5.1, §7.4 and §8.1: a
 * peer that breaks the protocol, sends a TEXT message or a CLOSE reason that is
 * not UTF-8, or a message larger than the server accepts is answered with a
 * CLOSE frame carrying a status code, and nothing more is sent.
 * fws_gpu_reply_messages_strict is fws_gpu_reply_messages_multi with that rule
 * applied on the device, from the verdicts the decode already left there; no
 * host walk of results and entries between decode and reply.
 *   dev_conn_states / conn_state_stride  the decode call's own state array, which
 *             the call only reads: fws_msg_carry records (stride 64) after
 *             fws_gpu_decode_messages_multi, fws_msg_flow records (stride 96,
 *             the carry first) after fws_gpu_decode_messages_flow; record
 *             dev_reads[r].conn is read r's.
 *   max_message_bytes  the largest message accepted, all its parts counted;
 *             0: no limit.
 * Every other argument, flags included, is fws_gpu_reply_messages_multi's, and
 * everything that call's contract says holds unchanged: the "no frames" cases,
 * the refusals and their order, bytes, records, states, max_len, ordering, no
 * workspace. A read with no failing item gets, byte for byte, what
 * fws_gpu_reply_messages_multi writes. What is added: each item of a read --
 * its n_msgs entries in order, then the open part, then, last, the decode's
 * error -- has a failure code or none, the first row that applies:
 *   TEXT / BIN entry  max_message_bytes > 0 and (prev_open_bytes of the state if
 *                     the entry is FWS_MSG_CONTINUED, else 0) + len exceeds it   1009
 *   TEXT entry        utf8_ok == 0                                                1007
 *   the open part     (judged whether or not open_len is 0) max_message_bytes > 0
 *                     and the state's open_bytes (stride 96: open_bytes +
 *                     frame_unread) exceeds it: a frame that announces too much
 *                     fails in the read that holds its header                    1009
 *   the open part     open_opcode == 1 and the state's utf8_bad is set: the early
 *                     failure §8.1 allows                                         1007
 *   CLOSE entry       len == 1                                                    1002
 *   CLOSE entry       len >= 2 and a status code outside 1000-1003, 1007-1014,
 *                     3000-4999 (the IANA registry as of RFC 6455 and 1012-1014;
 *                     1004-1006, 1015, anything below 1000, 1016-2999 and
 *                     anything from 5000 on may not appear in a frame)            1002
 *   CLOSE entry       len > 2 and bytes [2, len) are not well-formed UTF-8 as a
 *                     whole string (Unicode Table 3-7; a sequence cut by the end
 *                     is malformed)                                               1007
 *   the decode's error  status == FWS_ERR_TOO_LARGE                               1009
 *   the decode's error  status FWS_ERR_RSV, FWS_ERR_NOT_MASKED, FWS_ERR_MASKED,
 *                     FWS_ERR_OPCODE, FWS_ERR_CONTROL_FRAME or FWS_ERR_SEQUENCE   1002
 * Only the read's first CLOSE entry is judged, whatever flags is: with
 * FWS_REPLY_CONTROL nothing follows it, without it the CLOSE and what follows are
 * the host's. A CLOSE of length 0 or with a valid code and reason, a PING and a
 * PONG never fail. FWS_ERR_CAPACITY statuses, undelivered decodes and
 * FWS_ERR_DECLINED / FWS_ERR_INVALID reads are not failures and are treated as
 * by fws_gpu_reply_messages_multi.
 * Let f be the first failing item and c the first CLOSE entry answered (with
 * FWS_REPLY_CONTROL). With no f, or c < f, the read is answered as by
 * fws_gpu_reply_messages_multi. Otherwise the items before f are answered as
 * there; in f's place goes one CLOSE frame, FIN = 1, whose payload is the code's
 * two big-endian bytes (no reason), whatever flags is, 0 included; every later
 * item is dropped; dev_states[conn] gets close_sent = 1 and fail_code = the
 * code, and close_code as above if f was a CLOSE entry, else it is left as it
 * was. The open part is sent before the failing frame only when f is the
 * decode's error. A close_sent found set still means "no frames".
 *   capacity  the bytes and the frame count include the failing frame (4 bytes);
 *             on FWS_ERR_CAPACITY nothing is written and both states are intact.
 *   refusals  one more, tested just before FWS_ERR_CAPACITY: FWS_ERR_INVALID for
 *             more than FWS_MSG_MULTI_MAX_FRAMES + 2 frames (257 entries, an open
 *             part and an error: not a decode output).
 * The reference's server closes with 1006 and an error text on such errors
 * (ws_server_socket.h:176-181). RFC 6455 §7.4.1 reserves 1006 and forbids it in
 * a frame; this call follows the RFC. The FLoop hook, which reproduces the
 * reference's text, is untouched.
 * n == 0 returns 0 and looks at nothing. Otherwise the checks of
 * fws_gpu_reply_messages_multi apply, dev_conn_states must be non-null and
 * conn_state_stride 64 or 96, or the call returns FWS_ERR_INVALID before any
 * device call. A client's (masked) replies are
 * fws_gpu_reply_messages_strict_client's below. Out of scope: a reason in the
 * failing CLOSE; cutting a part into several frames; a limit per connection; stopping
 * the decode of a failed connection (the host drops it when it sees fail_code);
 * the C++ adapter and the FLoop hook. */
int fws_gpu_reply_messages_strict(fws_gpu_ctx *ctx,
                                  const fws_msg_read *dev_reads, uint32_t n, uint32_t max_len,
                                  const fws_msg_info *dev_msgs, const void *dev_dst, const void *dev_ctl,
                                  const fws_msg_result *dev_msg_results,
                                  const void *dev_conn_states, uint32_t conn_state_stride,
                                  uint64_t max_message_bytes,
                                  const fws_reply_region *dev_regions, void *dev_out,
                                  fws_frame_info *dev_frames, fws_tx_result *dev_results,
                                  fws_tx_conn *dev_conns, fws_reply_state *dev_states, uint32_t n_conns,
                                  uint32_t flags, void *stream);

/* ---- the same two calls for a client: masked replies ----------------------------
 * A client's frames carry the MASK bit and a key (SendFrame in the client role,
 * w_socket.h:857-871). fws_gpu_reply_messages_multi_client and
 * fws_gpu_reply_messages_strict_client are fws_gpu_reply_messages_multi and
 * fws_gpu_reply_messages_strict with one argument added between flags and
 * stream, and they answer what fws_gpu_decode_messages_flow_client delivered.
 *   dev_keys  device memory, one word per read: dev_keys[r] is read r's key. The
 *             call only reads it. NULL is FWS_ERR_INVALID before any device call
 *             (n == 0 still returns 0 and looks at nothing).
 * Everything in the two contracts above holds: the items and their order, the
 * "no frames" cases, the refusals and their order, both states, the strict
 * failure table, max_len, ordering, the absence of a workspace, no byte written
 * outside [out_off, out_off + out_len). What differs:
 *   bytes     every frame is a client frame: the MASK bit, 4 key bytes behind
 *             the length, the payload XORed with the key from phase 0 -- what
 *             fws_gpu_encode_frames writes for the same payload, opcode, FIN,
 *             masked = 1 and key. A header is 2 + 4 + (0 | 2 | 8) bytes.
 *   keys      frame j of read r uses FWS_TX_FRAG_KEY(dev_keys[r], j), as a masked
 *             send of fws_gpu_encode_messages_multi does. j counts the frames
 *             written to the region from 0, in order, the strict call's failing
 *             CLOSE included. (The reference draws a fresh random key per frame,
 *             w_socket.h:860; any key is as good, and the caller supplies the
 *             randomness per read.)
 *   records   fws_frame_info.key is the frame's key: the records are the ones
 *             fws_gpu_decode_messages_flow (the server role) reports for the
 *             same bytes.
 *   lengths   out_len, the FWS_ERR_CAPACITY test and wire_bytes count the 4 key
 *             bytes of every frame. The strict failing CLOSE is 8 bytes: header
 *             2, key 4, the code's 2 bytes masked.
 *   strict    conn_state_stride is 64 or 96 as before; after
 *             fws_gpu_decode_messages_flow_client it is 96.
 * Out of scope, as above: a reason in the failing CLOSE, cutting a part into
 * several frames, the C++ adapter and the FLoop hook. */
int fws_gpu_reply_messages_multi_client(fws_gpu_ctx *ctx,
                                        const fws_msg_read *dev_reads, uint32_t n, uint32_t max_len,
                                        const fws_msg_info *dev_msgs, const void *dev_dst, const void *dev_ctl,
                                        const fws_msg_result *dev_msg_results,
                                        const fws_reply_region *dev_regions, void *dev_out,
                                        fws_frame_info *dev_frames, fws_tx_result *dev_results,
                                        fws_tx_conn *dev_conns, fws_reply_state *dev_states, uint32_t n_conns,
                                        uint32_t flags, const uint32_t *dev_keys, void *stream);
int fws_gpu_reply_messages_strict_client(fws_gpu_ctx *ctx,
                                         const fws_msg_read *dev_reads, uint32_t n, uint32_t max_len,
                                         const fws_msg_info *dev_msgs, const void *dev_dst, const void *dev_ctl,
                                         const fws_msg_result *dev_msg_results,
                                         const void *dev_conn_states, uint32_t conn_state_stride,
                                         uint64_t max_message_bytes,
                                         const fws_reply_region *dev_regions, void *dev_out,
                                         fws_frame_info *dev_frames, fws_tx_result *dev_results,
                                         fws_tx_conn *dev_conns, fws_reply_state *dev_states, uint32_t n_conns,
                                         uint32_t flags, const uint32_t *dev_keys, void *stream);

/* ---- messages that span reads, joined on the device ------------------------------
 * The decode calls deliver a message that arrives over several reads as parts:
 * the open part of each call (open_off / open_len), then one FWS_MSG_CONTINUED
 * entry whose off / len describe the last part only, each part in the read's
 * region of dev_dst, which the next call overwrites. fws_gpu_join_messages puts
 * the parts together in device memory, so that a consumer on the device -- a
 * kernel that parses what arrives, a copy to the application's buffer -- sees
 * every message as one contiguous run of bytes. It reads what
 * fws_gpu_decode_messages_flow, _flow_client or _multi wrote for
 * dev_reads[0..n), one workgroup per read, and changes nothing in it. */
#define FWS_JOIN_IN_DST   0u   /* the message is whole in this read: dev_dst, not copied */
#define FWS_JOIN_IN_STORE 1u   /* joined in the connection's slot of dev_store */
#define FWS_JOIN_IN_CTL   2u   /* a control frame: dev_ctl */
#define FWS_JOIN_NOWHERE  3u   /* dropped: longer than half a slot */
#define FWS_JOIN_DROPPED  1u   /* fws_join_info.flags */

typedef struct fws_join_state {  /* device memory, one per connection; all zero = new */
    uint32_t open_opcode;        /* 0: none open; 1 / 2 */
    uint32_t half;               /* 0 / 1: the half of the slot the open (or next) joined message uses */
    uint32_t dropped;            /* 1: the open message outgrew its half; its bytes are not kept */
    uint32_t reserved0;          /* 0 */
    uint64_t open_bytes;         /* bytes of the open message seen so far, all calls */
    uint64_t fill;               /* bytes of it in the half (== open_bytes, or 0 when dropped) */
} fws_join_state;                /* 32 bytes */

typedef struct fws_join_info {   /* one per decode entry, same index */
    uint64_t off;                /* from the base of the buffer `where` names (absolute, not per read) */
    uint64_t len;                /* the whole message, all its parts */
    uint8_t opcode, utf8_ok, where, flags;
    uint32_t reserved0;
    uint64_t reserved;
} fws_join_info;                 /* 32 bytes */

typedef struct fws_join_result {
    int32_t status;
    uint32_t n_joined;           /* records written */
    uint64_t copied;             /* bytes this read put into dev_store */
    uint32_t open_opcode;        /* the state after the read */
    uint32_t dropped;
    uint64_t reserved;
} fws_join_result;               /* 32 bytes */

/* dev_reads, n, max_len, dev_msgs, dev_dst and dev_msg_results are the decode
 * call's own arguments; the call only reads them.
 *   slots     connection c's slot is dev_store + c * store_stride: two halves of
 *             H = store_stride / 2 bytes. A message of more than H bytes is
 *             dropped (below); a server that runs fws_gpu_reply_messages_strict
 *             with 0 < max_message_bytes <= H has already answered it with 1009.
 *   records   dev_joined[msg_base + i] describes entry dev_msgs[msg_base + i], i <
 *             n_msgs. A FWS_JOIN_IN_STORE message stays valid until the next
 *             fws_gpu_join_messages call that names the connection; a
 *             FWS_JOIN_IN_DST or FWS_JOIN_IN_CTL message as long as the decode's
 *             regions do.
 * Per read r (conn = dev_reads[r].conn, S = dev_states[conn]), the entries in
 * order, then the open part:
 *   1. a control entry: where = FWS_JOIN_IN_CTL, off = ctl_off + entry.off, len,
 *      opcode (utf8_ok 0). Nothing is copied.
 *   2. a data entry without FWS_MSG_CONTINUED: where = FWS_JOIN_IN_DST, off =
 *      dst_off + entry.off, len, opcode, utf8_ok. Nothing is copied.
 *   3. the data entry with FWS_MSG_CONTINUED (at most one, the read's first data
 *      entry): dev_dst[dst_off, dst_off + entry.len) is appended. Then, if
 *      S.dropped: where = FWS_JOIN_NOWHERE, off = 0, len = S.open_bytes, flags =
 *      FWS_JOIN_DROPPED, S.half unchanged; else where = FWS_JOIN_IN_STORE, off =
 *      conn * store_stride + S.half * H, len = S.fill, and S.half ^= 1. Either
 *      way opcode and utf8_ok are the entry's (the verdict on the whole message)
 *      and open_opcode, dropped, open_bytes and fill become 0.
 *   4. the open part, when fws_msg_result.open_opcode != 0: if S.open_opcode == 0
 *      a new message starts (S.open_opcode = open_opcode, dropped = open_bytes =
 *      fill = 0); then dev_dst[dst_off + open_off, + open_len) is appended
 *      (open_len may be 0).
 *   append p bytes: S.open_bytes += p; if S.dropped nothing is copied; else if
 *      S.fill + p > H then S.dropped = 1, S.fill = 0 and nothing of this part is
 *      copied; else the part goes to slot + S.half * H + S.fill and S.fill += p.
 * The half toggles when a joined message is delivered, so the message rule 3
 * delivers stays intact while rule 4 starts the next one in the other half, in
 * the same read.
 *   bytes     dev_store is written only inside the appended ranges: no byte
 *             before fill, no byte of the other half, no byte of another
 *             connection's slot. Loads touch only the 16-B aligned chunks of
 *             dev_dst that hold at least one byte of a part.
 *   nothing to do  status 0, n_joined 0, copied 0, the state untouched (the result's
 *             open_opcode / dropped echo it): the reply calls' "no frames" tests --
 *             the read's fws_msg_result.status is FWS_ERR_DECLINED or
 *             FWS_ERR_INVALID, or its decode delivered nothing (n_msgs > msg_cap,
 *             data_bytes > dst_cap or ctl_bytes > ctl_cap, the capacities taken
 *             from the read's descriptor). Every other status (0, a protocol or
 *             sequencing error, a frame-count FWS_ERR_CAPACITY) leaves a valid
 *             prefix, and that prefix is joined.
 *   refusals  per read; the call still returns 0, only the read's result is
 *             written (other fields zero), the state and dev_store are untouched.
 *             Tested in this order, before any store:
 *               FWS_ERR_INVALID   conn >= n_conns (before the "nothing to do" tests)
 *               FWS_ERR_INVALID   n_msgs > FWS_MSG_MULTI_MAX_FRAMES + 1
 *               FWS_ERR_INVALID   a data entry or the open part over
 *                                 FWS_MSG_MULTI_MAX_READ bytes, or S.open_opcode
 *                                 not 0, 1 or 2
 *               FWS_ERR_INVALID   decode and join out of step: a CONTINUED entry
 *                                 with S.open_opcode == 0; a CONTINUED entry that
 *                                 is not the first data entry; S.open_opcode != 0,
 *                                 no CONTINUED entry, and a data entry present or
 *                                 open_opcode != S.open_opcode
 *             A dropped message is not an error. Two reads of one call that name
 *             the same conn are a contract violation, as everywhere else.
 *   max_len   the decode call's value; it selects the workgroup form as there.
 *   ordering  stream-ordered: no host synchronisation, no copy, no allocation, no
 *             workspace. The call is queued behind its decode call and in front
 *             of the connection's next one, on either side of a reply call (both
 *             only read the decode's output). Calls chain through dev_states.
 * n == 0 returns 0 and looks at nothing. Otherwise ctx and every pointer must be
 * non-null, dev_dst and dev_store 16-B aligned, max_len between 1 and
 * FWS_MSG_MULTI_MAX_READ and store_stride a multiple of 32, at least 32, or the
 * call returns FWS_ERR_INVALID before any device call. Out of scope: joining
 * inside the decode kernels, a slot size per connection, echoing joined
 * messages, the C++ adapter and the FLoop hook. */
int fws_gpu_join_messages(fws_gpu_ctx *ctx,
                          const fws_msg_read *dev_reads, uint32_t n, uint32_t max_len,
                          const fws_msg_info *dev_msgs, const void *dev_dst,
                          const fws_msg_result *dev_msg_results,
                          void *dev_store, uint64_t store_stride,
                          fws_join_info *dev_joined, fws_join_result *dev_results,
                          fws_join_state *dev_states, uint32_t n_conns, void *stream);

/* ---- messages fanned out to many connections ------------------------------------
 * Every call above is one-to-one: what came from or goes to connection c stays
 * with connection c. fws_gpu_publish_messages is one-to-many: a set of messages
 * in device memory, lists of them, and per receiving connection (a subscriber)
 * one list and one region of dev_out, one workgroup per subscriber. A room's
 * members all name the room's list; each gets the listed messages as server
 * frames, back to back, several a call. The messages are fws_join_info records,
 * the layout fws_gpu_join_messages writes, so what a join call delivered is
 * published with no host in between; an application that publishes its own
 * payloads fills such records itself: where = FWS_JOIN_IN_DST and off from the
 * buffer it passes as dev_dst, FWS_JOIN_IN_STORE and dev_store, FWS_JOIN_IN_CTL
 * and dev_ctl. utf8_ok, flags and the reserved fields are not looked at. */
#define FWS_PUB_MAX_ITEMS 256u          /* records one subscriber's list may name */

typedef struct fws_pub_sub {            /* device memory, one per receiving connection */
    uint64_t out_off;                   /* its region of dev_out, 16-B aligned */
    uint32_t out_cap;
    uint32_t conn;                      /* index into dev_conns / dev_states, < n_conns; distinct within a call */
    uint32_t list_off, list_len;        /* its items: dev_list[list_off .. list_off + list_len) */
    uint32_t frame_base, frame_cap;     /* its slice of dev_frames (frame_cap 0: no records) */
} fws_pub_sub;                          /* 32 bytes */

/* dev_list holds n_list indices into dev_msgs[0..n_msgs); slices of it may be
 * shared by any number of subscribers and may overlap. Per subscriber s (conn =
 * dev_subs[s].conn, offsets relative to the region dev_out + out_off):
 *   items     the listed records in list order. A record with opcode == 0 or
 *             where == FWS_JOIN_NOWHERE is nothing: no frame, and not judged --
 *             so a caller that zeroes dev_joined on the stream before the join
 *             call may list every slot of a read's entry slice without knowing
 *             n_msgs. Opcode 1 or 2: one data frame with that opcode, FIN = 1,
 *             the whole message as payload (len 0: an empty frame). Opcode 9 or
 *             10: one control frame, FIN = 1. Opcode 8: one CLOSE frame with the
 *             record's payload; dev_states[conn].close_sent becomes 1, close_code
 *             and fail_code stay what they were, and every later item of the
 *             list is dropped (a server going away with 1001).
 *   bytes     server frames (no MASK bit, no key) back to back from the region's
 *             start, each what fws_gpu_encode_frames writes for that payload,
 *             opcode and FIN. No byte outside [out_off, out_off + out_len) is
 *             written, inside out_cap or not. Sources may have any alignment;
 *             loads touch only the 16-B aligned chunks of a source that hold at
 *             least one payload byte. Regions must not overlap each other or any
 *             source.
 *   state     on success dev_conns[conn] keeps last_msg_not_fin, frames +=
 *             n_frames, wire_bytes += out_len; dev_states[conn] as above. The
 *             result echoes last_msg_not_fin (as 0 / 1).
 *   records   dev_frames[frame_base + j], j < min(n_frames, frame_cap), as the
 *             reply calls write them (hdr_off relative to the region, key 0).
 *             dev_frames may be NULL when every frame_cap is 0.
 *   refusals  per subscriber; the call still returns 0, only the subscriber's
 *             result is written (other fields zero except where stated), both
 *             states and the region are untouched, and other subscribers are
 *             not affected. Every listed record that is not nothing is judged,
 *             dropped behind a CLOSE or not. The verdict is the first row that
 *             applies to any of them:
 *               FWS_ERR_INVALID        out_off not 16-B aligned, conn >= n_conns,
 *                                      list_len > FWS_PUB_MAX_ITEMS, list_off +
 *                                      list_len > n_list, an index >= n_msgs, an
 *                                      opcode not 0, 1, 2, 8, 9 or 10, a where
 *                                      above 3, a record (of any len) that names
 *                                      a base passed as NULL
 *               (no frames)            status 0, n_frames 0, out_len 0, the result
 *                                      echoes last_msg_not_fin: close_sent is set,
 *                                      or the list is empty or all nothing
 *               FWS_ERR_CONTROL_FRAME  an opcode 8, 9 or 10 record over 125 bytes
 *               FWS_ERR_DECLINED       a data record with len > max_len or len >
 *                                      FWS_TX_MULTI_MAX_SEND: the host sends such a
 *                                      message in pieces through
 *                                      fws_gpu_encode_messages_multi
 *               FWS_ERR_SEQUENCE       dev_conns[conn].last_msg_not_fin != 0 and a
 *                                      data frame is among the frames that would
 *                                      be written: the application is in the
 *                                      middle of a fragmented send to this
 *                                      connection, and a whole message must not
 *                                      be cut into it. (The reference's SendFrame
 *                                      would silently make it a continuation,
 *                                      w_socket.h:845-848; this call refuses
 *                                      instead.) A control-only list, or one
 *                                      whose data records all lie behind a CLOSE,
 *                                      goes through and leaves last_msg_not_fin
 *                                      as it was.
 *               FWS_ERR_CAPACITY       the bytes needed exceed out_cap; out_len =
 *                                      the bytes needed, n_frames is set
 *             Two subscribers of one call that name the same conn are a contract
 *             violation: the result is undefined for that connection only.
 *   max_len   the caller's bound on a data record's len, between 1 and
 *             FWS_TX_MULTI_MAX_SEND. It selects the workgroup form as in the reply
 *             calls: up to 16 KiB 256 threads, above 1024.
 *   ordering  stream-ordered: no host synchronisation, no copy, no allocation, no
 *             workspace. Calls queued on one stream chain through dev_conns and
 *             dev_states; a publish call may stand on either side of a reply or
 *             encode call that shares them.
 * n == 0 returns 0 and looks at nothing. Otherwise ctx, dev_msgs, dev_list,
 * dev_subs, dev_out, dev_results, dev_conns and dev_states must be non-null,
 * dev_out 16-B aligned and max_len in range, or the call returns FWS_ERR_INVALID
 * before any device call; dev_dst, dev_store, dev_ctl and dev_frames may be NULL.
 * A region is at most FWS_PUB_MAX_ITEMS * (FWS_TX_MULTI_MAX_SEND + 10) bytes,
 * below 2^26. Out of scope: cutting a message into several frames; masked
 * (client) frames; leaving the sender out of its own room (the host builds the
 * lists); dropping TEXT records with utf8_ok == 0; topic-major input (message ->
 * subscribers) and its inversion on the device; the C++ adapter and the FLoop
 * hook. */
int fws_gpu_publish_messages(fws_gpu_ctx *ctx,
                             const fws_join_info *dev_msgs, uint32_t n_msgs,
                             const void *dev_dst, const void *dev_store, const void *dev_ctl,
                             const uint32_t *dev_list, uint32_t n_list,
                             const fws_pub_sub *dev_subs, uint32_t n, uint32_t max_len,
                             void *dev_out, fws_frame_info *dev_frames, fws_tx_result *dev_results,
                             fws_tx_conn *dev_conns, fws_reply_state *dev_states, uint32_t n_conns, void *stream);

/* Host-memory send for one connection: WSocket::SendFrame (w_socket.h:832-944)
 * for its next n frames, in order. Frame i = payloads[i][0..lens[i]) of
 * WSTxFrameType frame_types[i] with last_frame_if_possible = last[i]; a client
 * session (is_server = 0) masks with keys[i] (the reference draws
 * SemiSecureRand32, w_socket.h:860; here the caller supplies it). The frames'
 * wire bytes, back to back, go to out; *out_len = their size. If out_cap is
 * too small: FWS_ERR_CAPACITY, *out_len = the size needed, nothing sent and
 * the sequencing state unchanged. Opcode / FIN sequencing (last_msg_not_fin_,
 * w_socket.h:903-913) is carried across calls. Synchronous; empty control
 * payloads are sent as empty frames (the reference dereferences a null
 * buffer there). */
typedef struct fws_tx_session fws_tx_session;
int fws_tx_session_create(fws_gpu_ctx *ctx, int is_server, fws_tx_session **out);
void fws_tx_session_destroy(fws_tx_session *s);
int fws_tx_session_send(fws_tx_session *s, const uint8_t *const *payloads, const uint64_t *lens,
                        const uint32_t *frame_types, const uint8_t *last, const uint32_t *keys, uint32_t n,
                        uint8_t *out, uint64_t out_cap, uint64_t *out_len);
int fws_tx_session_state(const fws_tx_session *s, uint8_t *last_msg_not_fin);

/* ---- batched, pipelined receive over host memory ---------------------------
 * the reads of one event-loop step (FLoop::OneStep,
 * floop.h:661-703; TCPSocket::Read, tcp_socket.h:387-402) aggregated into one
 * host batch per submit. Each of `depth` slots runs H2D -> decode (header parse
 * + unmask, optional per-frame UTF-8 flags) -> D2H of the unmasked bytes (back
 * into the batch), the frame list and the result on its own stream, so
 * successive batches overlap on the full-duplex link. The batch must stay
 * valid (and should be pinned) until its wait returns; a batch starts at a
 * frame header (the per-connection carry is the session's job). */
typedef struct fws_rx_pipe fws_rx_pipe;

/* Pin / unpin caller memory (e.g. MemPool blocks, flash_alloc.h:44-73) for async copies. */
int fws_gpu_host_register(void *host_ptr, uint64_t bytes);
int fws_gpu_host_unregister(void *host_ptr);

int fws_rx_pipe_create(int device, uint64_t max_batch_bytes, uint32_t max_frames, uint32_t depth, int utf8,
                       fws_rx_pipe **out);
void fws_rx_pipe_destroy(fws_rx_pipe *p);
/* Enqueue a batch; *ticket identifies it. Waits first if its slot is still busy. */
int fws_rx_pipe_submit(fws_rx_pipe *p, uint8_t *batch, uint64_t len, uint64_t *ticket);
/* Block until batch `ticket` is done: the batch holds the unmasked bytes, *frames
 * points at min(n_frames, max_frames) decoded frames (pinned, valid until the
 * slot is reused `depth` submits later), *result is the decode result, and
 * *utf8_ok the per-frame flags (pipes created with utf8 != 0). */
int fws_rx_pipe_wait(fws_rx_pipe *p, uint64_t ticket, const fws_frame_info **frames, uint64_t *n_frames,
                     fws_decode_result *result, const uint8_t **utf8_ok);

/* ---- synthetic workloads (BASELINE configs, not test oracles) ------------ */
typedef struct fws_gen_params {
    uint64_t seed;
    uint32_t kind;          /* 0 fixed-size frames, 1 log-uniform sizes, 2 fragmented message, 3 UTF-8 text */
    uint32_t opcode;        /* data opcode for kinds 0/1 (1 TEXT, 2 BIN) */
    uint64_t n_frames;      /* kinds 0/3: frame count */
    uint64_t payload_min;   /* kind 0/3: the payload size; kinds 1/2: minimum */
    uint64_t payload_max;   /* kinds 1/2: maximum (log-uniform in [min, max]) */
    uint64_t target_bytes;  /* kinds 1/2: stop once the payload total reaches this */
    uint32_t invalid_permille; /* kind 3: frames carrying one invalid UTF-8 sequence */
    uint32_t pad_;
} fws_gen_params;

/* Two-call protocol: with wire == NULL only *wire_len and *n_frames are
 * computed. Otherwise fills wire (cap bytes, host memory) with client-masked
 * frames and descs (payload regions, phase 0) and, for kind 3, utf8_ok
 * (expected per-frame validity). */
int fws_gen_batch(const fws_gen_params *p, uint8_t *wire, uint64_t cap, uint64_t *wire_len,
                  fws_frame_desc *descs, uint64_t descs_cap, uint64_t *n_frames, uint8_t *utf8_ok);

#ifdef __cplusplus
}
#endif
#endif /* FWS_GPU_H */
