"""Python face of the MI355X decode path, mirroring the reference's interface
for this path (names and argument meaning of crypto/ws_mask.h and
net/w_socket.h, error codes of ParseFrameHdr). Device memory, streams and
events come from torch; all compute runs in libfws_gpu.so's HIP kernels.
"""
import ctypes as C
import random

import numpy as np
import torch

from . import _lib
from ._lib import (DECODE_JOB, FRAME_DESC, FRAME_INFO, DECODE_RESULT, MSG_CARRY, MSG_INFO, MSG_READ, MSG_RESULT,
                   RX_EVENT, TX_DESC, FwsError, GenParams, check, lib)


def _stream_handle(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


_hip = None


def hip_stream():
    """A HIP stream created with hipStreamNonBlocking, as the library's own
    pipelines create theirs (rx_pipe.cpp, rx_session.cpp), wrapped for torch.
    Two of these overlap two decodes every time; two torch pool streams did so
    only in some runs (tools/stream_pair_probe.py: 165-171 vs 176-208 us per
    C3 batch)."""
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
    s = C.c_void_p()
    if _hip.hipStreamCreateWithFlags(C.byref(s), C.c_uint(1)) != 0:
        raise RuntimeError("hipStreamCreateWithFlags failed")
    return HipStream(s.value)


class HipStream(torch.cuda.ExternalStream):
    """A stream from hip_stream(); close() (or leaving a `with` block)
    synchronizes and destroys it, so probes that make fresh pairs do not leak
    streams and their queue bindings."""

    def close(self):
        h = self.cuda_stream
        if h and _hip is not None and not getattr(self, "_closed", False):
            self._closed = True
            _hip.hipStreamSynchronize(C.c_void_p(h))
            _hip.hipStreamDestroy(C.c_void_p(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def device_count():
    n = C.c_int(0)
    check("fws_gpu_device_count", lib().fws_gpu_device_count(C.byref(n)))
    return n.value


class Ctx:
    """fws_gpu_ctx: device workspace for one device / one host thread."""

    def __init__(self, device=0, max_frames=0, max_stream_bytes=0):
        self.device = device
        h = C.c_void_p()
        check("fws_gpu_ctx_create", lib().fws_gpu_ctx_create(device, C.byref(h)))
        self.h = h
        if max_frames or max_stream_bytes:
            self.reserve(max_frames, max_stream_bytes)

    def reserve(self, max_frames, max_stream_bytes):
        check("fws_gpu_ctx_reserve", lib().fws_gpu_ctx_reserve(self.h, max_frames, max_stream_bytes))

    def set_rx_persistent(self, workers):
        """fws_gpu_ctx_set_rx_persistent: the context's small reads decoded by a
        resident grid of `workers` workgroups (0 = a launch per read)."""
        check("fws_gpu_ctx_set_rx_persistent", lib().fws_gpu_ctx_set_rx_persistent(self.h, workers))

    def rx_service_stats(self):
        """(grid launches, requests) of the persistent receive decode"""
        out = (C.c_uint64 * 2)()
        check("fws_internal_rx_service_stats", lib().fws_internal_rx_service_stats(self.h, out))
        return int(out[0]), int(out[1])

    def rx_service_pushes(self):
        """reads the persistent decode took pushed into device memory (push mode)"""
        out = (C.c_uint64 * 1)()
        check("fws_internal_rx_service_pushes", lib().fws_internal_rx_service_pushes(self.h, out))
        return int(out[0])

    def close(self):
        if self.h:
            lib().fws_gpu_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ws_mask_bytes_fast(buf, key, offset=0, n=None, stream=None):
    """Device twin of fws::WSMaskBytesFast(src, size, mask) (ws_mask.h:175):
    XOR buf[offset:offset+n] (a uint8 CUDA tensor) with the 4-byte key in place."""
    n = buf.numel() - offset if n is None else n
    check("fws_gpu_mask", lib().fws_gpu_mask(C.c_void_p(buf.data_ptr() + offset), n, key & 0xFFFFFFFF,
                                             _stream_handle(stream)))


def descs_to_device(descs, device="cuda"):
    """numpy FRAME_DESC array -> uint8 device tensor holding the structs."""
    a = np.ascontiguousarray(descs, dtype=FRAME_DESC)
    return torch.from_numpy(a.view(np.uint8)).to(device)


def unmask_batch(ctx, base, dev_descs, n, stream=None):
    """fws_gpu_unmask_batch: unmask every payload region in place."""
    check("fws_gpu_unmask_batch", lib().fws_gpu_unmask_batch(ctx.h, _ptr(base), _ptr(dev_descs), n,
                                                             _stream_handle(stream)))


def unmask_sorted(ctx, base, dev_descs, n, stream=None):
    """fws_gpu_unmask_sorted: one-launch unmask of a sorted, non-overlapping batch."""
    check("fws_gpu_unmask_sorted", lib().fws_gpu_unmask_sorted(ctx.h, _ptr(base), _ptr(dev_descs), n,
                                                               _stream_handle(stream)))


def unmask_sorted_utf8(ctx, base, dev_descs, n, ok, stream=None):
    """fws_gpu_unmask_sorted_utf8: one-pass unmask + per-region UTF-8 flags (ok: device uint8[n])."""
    check("fws_gpu_unmask_sorted_utf8", lib().fws_gpu_unmask_sorted_utf8(ctx.h, _ptr(base), _ptr(dev_descs), n,
                                                                         _ptr(ok), _stream_handle(stream)))


def unmask_plan(ctx, base, dev_descs, n, stream=None):
    check("fws_gpu_unmask_plan", lib().fws_gpu_unmask_plan(ctx.h, _ptr(base), _ptr(dev_descs), n,
                                                           _stream_handle(stream)))


def unmask_run(ctx, base, dev_descs, n, stream=None):
    check("fws_gpu_unmask_run", lib().fws_gpu_unmask_run(ctx.h, _ptr(base), _ptr(dev_descs), n,
                                                         _stream_handle(stream)))


def unmask_gather(ctx, dst, src, dev_descs, n, stream=None):
    check("fws_gpu_unmask_gather", lib().fws_gpu_unmask_gather(ctx.h, _ptr(dst), _ptr(src), _ptr(dev_descs),
                                                               n, _stream_handle(stream)))


def decode_stream(ctx, wire, cap, frames=None, result=None, utf8_ok=None, stream=None, n=None):
    """fws_gpu_decode_stream on a device uint8 tensor. Returns (status, frames
    tensor, result tensor, utf8 tensor) -- device tensors, nothing synchronised."""
    dev = wire.device
    if frames is None:
        frames = torch.empty(max(cap, 1) * FRAME_INFO.itemsize, dtype=torch.uint8, device=dev)
    if result is None:
        result = torch.empty(DECODE_RESULT.itemsize, dtype=torch.uint8, device=dev)
    n = wire.numel() if n is None else n
    u = C.c_void_p(utf8_ok.data_ptr()) if utf8_ok is not None else None
    rc = lib().fws_gpu_decode_stream(ctx.h, _ptr(wire), n, _ptr(frames), cap, _ptr(result), u,
                                     _stream_handle(stream))
    return rc, frames, result, utf8_ok


def decode_messages(ctx, wire, cap, msg_cap, dst, ctl, frames=None, msgs=None, result=None, msg_result=None,
                    stream=None, n=None, dst_cap=None, ctl_cap=None):
    """fws_gpu_decode_messages on a device uint8 tensor: the stream's frames
    grouped into messages, data payloads unmasked into dst (16-B aligned),
    control payloads into ctl; wire is not modified. dst_cap / ctl_cap default
    to the tensors' sizes. Returns (status, frames, msgs, result, msg_result)
    -- device tensors, nothing synchronised."""
    dev = wire.device
    if frames is None:
        frames = torch.empty(max(cap, 1) * FRAME_INFO.itemsize, dtype=torch.uint8, device=dev)
    if msgs is None:
        msgs = torch.empty(max(msg_cap, 1) * MSG_INFO.itemsize, dtype=torch.uint8, device=dev)
    if result is None:
        result = torch.empty(DECODE_RESULT.itemsize, dtype=torch.uint8, device=dev)
    if msg_result is None:
        msg_result = torch.empty(MSG_RESULT.itemsize, dtype=torch.uint8, device=dev)
    n = wire.numel() if n is None else n
    dst_cap = dst.numel() if dst_cap is None else dst_cap
    ctl_cap = ctl.numel() if ctl_cap is None else ctl_cap
    rc = lib().fws_gpu_decode_messages(ctx.h, _ptr(wire), n, _ptr(frames), cap, _ptr(msgs), msg_cap, _ptr(dst),
                                       dst_cap, _ptr(ctl), ctl_cap, _ptr(result), _ptr(msg_result),
                                       _stream_handle(stream))
    return rc, frames, msgs, result, msg_result


def read_msg_result(msg_result):
    return np.frombuffer(msg_result.cpu().numpy().tobytes(), dtype=MSG_RESULT)[0]


def read_messages(msgs, count):
    raw = msgs[:count * MSG_INFO.itemsize].cpu().numpy()
    return np.frombuffer(raw.tobytes(), dtype=MSG_INFO).copy()


def decode_messages_carry(ctx, wire, cap, msg_cap, dst, ctl, carry, frames=None, msgs=None, result=None,
                          msg_result=None, stream=None, n=None, dst_cap=None, ctl_cap=None):
    """fws_gpu_decode_messages_carry: decode_messages for one read of a
    connection. carry is the connection's fws_msg_carry, a 64-byte device uint8
    tensor (zeros for a new connection) that the call reads and rewrites on the
    stream; wire holds the bytes from the previous call's resume_off on.
    Returns (status, frames, msgs, result, msg_result) -- device tensors,
    nothing synchronised."""
    dev = wire.device
    if frames is None:
        frames = torch.empty(max(cap, 1) * FRAME_INFO.itemsize, dtype=torch.uint8, device=dev)
    if msgs is None:
        msgs = torch.empty(max(msg_cap, 1) * MSG_INFO.itemsize, dtype=torch.uint8, device=dev)
    if result is None:
        result = torch.empty(DECODE_RESULT.itemsize, dtype=torch.uint8, device=dev)
    if msg_result is None:
        msg_result = torch.empty(MSG_RESULT.itemsize, dtype=torch.uint8, device=dev)
    n = wire.numel() if n is None else n
    dst_cap = dst.numel() if dst_cap is None else dst_cap
    ctl_cap = ctl.numel() if ctl_cap is None else ctl_cap
    rc = lib().fws_gpu_decode_messages_carry(ctx.h, _ptr(wire), n, _ptr(frames), cap, _ptr(msgs), msg_cap,
                                             _ptr(dst), dst_cap, _ptr(ctl), ctl_cap, _ptr(result),
                                             _ptr(msg_result), _ptr(carry), _stream_handle(stream))
    return rc, frames, msgs, result, msg_result


def read_msg_carry(carry):
    return np.frombuffer(carry.cpu().numpy().tobytes(), dtype=MSG_CARRY)[0]


class MessageStream:
    """One connection's reads turned into its messages and control frames: the
    caller's side of fws_gpu_decode_messages_carry in its reference form.

    feed(data) puts the bytes the previous call left (from its resume_off on:
    an unfinished frame) in front of data, makes one carry call and one
    synchronisation, and returns the units that call completed, in order, as
    (opcode, bytes, utf8_ok) -- utf8_ok is the verdict of a TEXT message, False
    otherwise. A message that arrives over several reads is delivered once,
    at its FIN frame, its parts joined; the parts are kept on the host, the
    wire bytes of a finished frame are never kept. max_read bounds one feed,
    max_frame a frame's header and payload (a frame must fit in the buffer).
    The buffers are sized so that no capacity can be exceeded. A protocol or
    sequencing error is left in `status`; the units before it are returned and
    a later feed raises."""

    def __init__(self, ctx, max_read, max_frame=1 << 16, device="cuda:0"):
        self.ctx = ctx
        self.max_read = max_read
        self.wire_cap = (max_read + max_frame + 15) & ~15
        self.cap = self.wire_cap // 6 + 1            # a client frame is at least 6 bytes
        dev = torch.device(device)
        u8 = dict(dtype=torch.uint8, device=dev)
        self.wire = torch.zeros(self.wire_cap, **u8)
        self.dst = torch.zeros(self.wire_cap, **u8)
        self.ctl = torch.zeros(self.wire_cap, **u8)
        self.frames = torch.zeros(self.cap * FRAME_INFO.itemsize, **u8)
        self.msgs = torch.zeros(self.cap * MSG_INFO.itemsize, **u8)
        self.result = torch.zeros(DECODE_RESULT.itemsize, **u8)
        self.msg_result = torch.zeros(MSG_RESULT.itemsize, **u8)
        self.carry = torch.zeros(MSG_CARRY.itemsize, **u8)
        pin = dict(dtype=torch.uint8, pin_memory=True)
        self._h_wire = torch.zeros(self.wire_cap, **pin)
        self._h_dst = torch.zeros(self.wire_cap, **pin)
        self._h_ctl = torch.zeros(self.wire_cap, **pin)
        self._h_msgs = torch.zeros(self.cap * MSG_INFO.itemsize, **pin)
        self._h_res = torch.zeros(MSG_RESULT.itemsize, **pin)
        self._pending = b""
        self._parts = []
        self.status = 0

    def feed(self, data):
        if self.status not in (0, _lib.FWS_ERR_CAPACITY):
            raise FwsError("MessageStream.feed after an error", self.status)
        data = bytes(data)
        if len(data) > self.max_read:
            raise ValueError(f"a read of {len(data)} bytes exceeds max_read = {self.max_read}")
        buf = self._pending + data
        n = len(buf)
        if n > self.wire_cap:
            raise ValueError("a frame exceeds max_frame: the unfinished frame and the read do not fit the buffer")
        ne = n // 6 + 1
        stream = torch.cuda.current_stream(self.wire.device)
        self._h_wire[:n] = torch.frombuffer(bytearray(buf), dtype=torch.uint8) if n else self._h_wire[:0]
        self.wire[:n].copy_(self._h_wire[:n], non_blocking=True)
        rc, *_ = decode_messages_carry(self.ctx, self.wire, self.cap, self.cap, self.dst, self.ctl, self.carry,
                                       frames=self.frames, msgs=self.msgs, result=self.result,
                                       msg_result=self.msg_result, stream=stream, n=n)
        check("fws_gpu_decode_messages_carry", rc)
        self._h_res.copy_(self.msg_result, non_blocking=True)
        self._h_msgs[:ne * MSG_INFO.itemsize].copy_(self.msgs[:ne * MSG_INFO.itemsize], non_blocking=True)
        self._h_dst[:n].copy_(self.dst[:n], non_blocking=True)
        self._h_ctl[:n].copy_(self.ctl[:n], non_blocking=True)
        stream.synchronize()
        r = np.frombuffer(self._h_res.numpy().tobytes(), dtype=MSG_RESULT)[0]
        entries = np.frombuffer(self._h_msgs.numpy()[:int(r["n_msgs"]) * MSG_INFO.itemsize].tobytes(), dtype=MSG_INFO)
        dst, ctl = self._h_dst.numpy(), self._h_ctl.numpy()
        units = []
        for e in entries:
            off, ln = int(e["off"]), int(e["len"])
            if e["opcode"] >= 8:
                units.append((int(e["opcode"]), ctl[off:off + ln].tobytes(), False))
                continue
            body = dst[off:off + ln].tobytes()
            if e["flags"] & _lib.FWS_MSG_CONTINUED:
                body = b"".join(self._parts) + body
            self._parts = []
            units.append((int(e["opcode"]), body, bool(e["utf8_ok"])))
        if int(r["open_opcode"]) and int(r["open_len"]):
            off = int(r["open_off"])
            self._parts.append(dst[off:off + int(r["open_len"])].tobytes())
        self._pending = buf[int(r["resume_off"]):]
        self.status = int(r["status"])
        return units


def decode_messages_multi(ctx, wire, reads, n, max_len, frames, msgs, dst, ctl, results, msg_results, carries,
                          n_conns, stream=None):
    """fws_gpu_decode_messages_multi: the reads of many connections in one
    launch. reads holds n fws_msg_read descriptors (_lib.MSG_READ) in a device
    uint8 tensor; every other argument is the device uint8 tensor the
    descriptors' offsets and slices refer to, results / msg_results n records
    each, carries n_conns fws_msg_carry records. Returns the call's status --
    per-read outcomes are in msg_results; nothing is synchronised."""
    return lib().fws_gpu_decode_messages_multi(ctx.h, _ptr(wire), _ptr(reads), n, max_len, _ptr(frames), _ptr(msgs),
                                               _ptr(dst), _ptr(ctl), _ptr(results), _ptr(msg_results),
                                               _ptr(carries), n_conns, _stream_handle(stream))


class MessageMux:
    """MessageStream for many connections: feed({conn: bytes, ...}) makes one
    fws_gpu_decode_messages_multi call and one synchronisation for all of them
    and returns {conn: [(opcode, bytes, utf8_ok), ...]}, the units each
    connection completed, in order. Per connection the host protocol is
    MessageStream's: the bytes from resume_off on are kept in front of the next
    read, the parts of a message that arrives over several reads are joined at
    its FWS_MSG_CONTINUED entry. A read the one-launch form declines (over
    _lib.FWS_MSG_MULTI_MAX_FRAMES headers) goes through decode_messages_carry
    with that connection's carry. A connection whose status is a protocol or
    sequencing error keeps it in status[conn]; feeding it again raises, the
    others go on. max_read bounds one connection's feed, max_frame a frame."""

    def __init__(self, ctx, n_conns, max_read, max_frame=1 << 16, device="cuda:0"):
        self.ctx, self.n_conns, self.max_read = ctx, n_conns, max_read
        self.slot = (max_read + max_frame + 15) & ~15
        if self.slot > _lib.FWS_MSG_MULTI_MAX_READ:
            raise ValueError("max_read + max_frame exceeds FWS_MSG_MULTI_MAX_READ")
        self.cap = min(self.slot // 6 + 1, _lib.FWS_MSG_MULTI_MAX_FRAMES)
        self.dev = torch.device(device)
        u8 = dict(dtype=torch.uint8, device=self.dev)
        pin = dict(dtype=torch.uint8, pin_memory=True)
        self._sizes = dict(wire=self.slot, dst=self.slot, ctl=self.slot, frames=self.cap * FRAME_INFO.itemsize,
                           msgs=self.cap * MSG_INFO.itemsize, res=DECODE_RESULT.itemsize, mres=MSG_RESULT.itemsize,
                           reads=MSG_READ.itemsize)
        self._d = {k: torch.zeros(n_conns * sz, **u8) for k, sz in self._sizes.items()}
        self._h = {k: torch.zeros(n_conns * sz, **pin) for k, sz in self._sizes.items()}
        self.carries = torch.zeros(n_conns * MSG_CARRY.itemsize, **u8)
        self._single = None
        self._pending = [b""] * n_conns
        self._parts = [[] for _ in range(n_conns)]
        self.status = [0] * n_conns

    def _fallback(self, conn, buf):
        """A declined read: the carry call on the same bytes with the connection's carry."""
        if self._single is None:
            self._single = MessageStream(self.ctx, self.max_read, self.slot - self.max_read - 15, device=self.dev)
        ms = self._single
        csz = MSG_CARRY.itemsize
        ms.carry.copy_(self.carries[conn * csz:(conn + 1) * csz])
        ms._pending, ms._parts, ms.status = buf, self._parts[conn], 0
        units = ms.feed(b"")
        self.carries[conn * csz:(conn + 1) * csz].copy_(ms.carry)
        self._pending[conn], self._parts[conn], self.status[conn] = ms._pending, ms._parts, ms.status
        return units

    def feed(self, reads):
        for conn, data in reads.items():
            if not 0 <= conn < self.n_conns:
                raise ValueError(f"connection {conn} out of range")
            if self.status[conn] not in (0, _lib.FWS_ERR_CAPACITY):
                raise FwsError(f"MessageMux.feed after an error on connection {conn}", self.status[conn])
            if len(data) > self.max_read:
                raise ValueError(f"a read of {len(data)} bytes exceeds max_read = {self.max_read}")
        conns = list(reads)
        n = len(conns)
        if n == 0:
            return {}
        bufs = [self._pending[c] + bytes(reads[c]) for c in conns]
        if max(map(len, bufs)) > self.slot:
            raise ValueError("a frame exceeds max_frame: the unfinished frame and the read do not fit the buffer")
        sz, hw = self._sizes, self._h["wire"].numpy()
        desc = np.zeros(n, dtype=MSG_READ)
        for i, (c, buf) in enumerate(zip(conns, bufs)):
            hw[i * self.slot:i * self.slot + len(buf)] = np.frombuffer(buf, dtype=np.uint8)
            desc[i] = (i * self.slot, i * self.slot, i * self.slot, len(buf), c, self.slot, self.slot,
                       i * self.cap, self.cap, i * self.cap, self.cap, 0)
        self._h["reads"].numpy()[:n * sz["reads"]] = desc.view(np.uint8)
        stream = torch.cuda.current_stream(self.dev)
        for k in ("wire", "reads"):
            self._d[k][:n * sz[k]].copy_(self._h[k][:n * sz[k]], non_blocking=True)
        max_len = max(1, max(map(len, bufs)))
        d = self._d
        check("fws_gpu_decode_messages_multi",
              decode_messages_multi(self.ctx, d["wire"], d["reads"], n, max_len, d["frames"], d["msgs"], d["dst"],
                                    d["ctl"], d["res"], d["mres"], self.carries, self.n_conns, stream=stream))
        for k in ("mres", "msgs", "dst", "ctl"):
            self._h[k][:n * sz[k]].copy_(d[k][:n * sz[k]], non_blocking=True)
        stream.synchronize()
        mres = np.frombuffer(self._h["mres"].numpy()[:n * sz["mres"]].tobytes(), dtype=MSG_RESULT)
        out = {}
        for i, (c, buf) in enumerate(zip(conns, bufs)):
            r = mres[i]
            if int(r["status"]) == _lib.FWS_ERR_DECLINED:
                out[c] = self._fallback(c, buf)
                continue
            entries = np.frombuffer(self._h["msgs"].numpy()[i * sz["msgs"]:i * sz["msgs"] + int(r["n_msgs"]) *
                                                            MSG_INFO.itemsize].tobytes(), dtype=MSG_INFO)
            dst = self._h["dst"].numpy()[i * self.slot:(i + 1) * self.slot]
            ctl = self._h["ctl"].numpy()[i * self.slot:(i + 1) * self.slot]
            units = []
            for e in entries:
                off, ln = int(e["off"]), int(e["len"])
                if e["opcode"] >= 8:
                    units.append((int(e["opcode"]), ctl[off:off + ln].tobytes(), False))
                    continue
                body = dst[off:off + ln].tobytes()
                if e["flags"] & _lib.FWS_MSG_CONTINUED:
                    body = b"".join(self._parts[c]) + body
                self._parts[c] = []
                units.append((int(e["opcode"]), body, bool(e["utf8_ok"])))
            if int(r["open_opcode"]) and int(r["open_len"]):
                off = int(r["open_off"])
                self._parts[c].append(dst[off:off + int(r["open_len"])].tobytes())
            self._pending[c] = buf[int(r["resume_off"]):]
            self.status[c] = int(r["status"])
            out[c] = units
        return out


def decode_messages_flow(ctx, wire, reads, n, max_len, frames, msgs, dst, ctl, results, msg_results, flows,
                         n_conns, stream=None):
    """fws_gpu_decode_messages_flow: decode_messages_multi with a state per
    connection that also holds a data frame in progress, so a read may begin
    and end inside a frame's payload. flows holds n_conns fws_msg_flow records
    (_lib.MSG_FLOW, zeros for new connections) in a device uint8 tensor; the
    other arguments are decode_messages_multi's. Returns the call's status;
    nothing is synchronised."""
    return lib().fws_gpu_decode_messages_flow(ctx.h, _ptr(wire), _ptr(reads), n, max_len, _ptr(frames), _ptr(msgs),
                                              _ptr(dst), _ptr(ctl), _ptr(results), _ptr(msg_results),
                                              _ptr(flows), n_conns, _stream_handle(stream))


def decode_messages_flow_client(ctx, wire, reads, n, max_len, frames, msgs, dst, ctl, results, msg_results, flows,
                                n_conns, stream=None):
    """fws_gpu_decode_messages_flow_client: decode_messages_flow in the client
    role. The reads hold server frames: no MASK bit (a masked frame is
    FWS_ERR_MASKED), headers of 2, 4 or 10 bytes, payload copied as it is. The
    arguments and the state tensor are decode_messages_flow's; one connection's
    state belongs to one role. Returns the call's status; nothing is
    synchronised."""
    return lib().fws_gpu_decode_messages_flow_client(ctx.h, _ptr(wire), _ptr(reads), n, max_len, _ptr(frames),
                                                     _ptr(msgs), _ptr(dst), _ptr(ctl), _ptr(results),
                                                     _ptr(msg_results), _ptr(flows), n_conns, _stream_handle(stream))


def read_msg_flow(flows, conn=0):
    sz = _lib.MSG_FLOW.itemsize
    return np.frombuffer(flows[conn * sz:(conn + 1) * sz].cpu().numpy().tobytes(), dtype=_lib.MSG_FLOW)[0]


class MessageFlow:
    """MessageMux without a frame limit: feed({conn: bytes, ...}) makes one
    fws_gpu_decode_messages_flow call and one synchronisation for all
    connections and returns {conn: [(opcode, bytes, utf8_ok), ...]}, the units
    each connection completed, in order. A data frame's payload is decoded as
    it arrives, so a frame may be of any size and is uploaded once; what is
    kept in front of the next read is at most a partial header or a cut control
    frame (_lib.FWS_MSG_FLOW_MAX_PENDING bytes). The parts of a message that
    arrives over several reads are joined at its FWS_MSG_CONTINUED entry. A
    read with more headers than one call takes (FWS_ERR_CAPACITY with
    progress) is continued from resume_off by further calls for that
    connection inside the same feed; there is no other path. A connection
    whose status is a protocol or sequencing error keeps it in status[conn];
    feeding it again raises, the others go on. max_read bounds one
    connection's feed. role="client" decodes what a client receives (server
    frames, fws_gpu_decode_messages_flow_client); a frame is then as short as 2
    bytes and the frame slices are sized for that."""

    def __init__(self, ctx, n_conns, max_read, device="cuda:0", role="server"):
        if role not in ("server", "client"):
            raise ValueError(f"role must be 'server' or 'client', not {role!r}")
        self.ctx, self.n_conns, self.max_read, self.role = ctx, n_conns, max_read, role
        self._decode = decode_messages_flow_client if role == "client" else decode_messages_flow
        self._decode_name = "fws_gpu_decode_messages_flow" + ("_client" if role == "client" else "")
        if max_read + _lib.FWS_MSG_FLOW_MAX_PENDING > _lib.FWS_MSG_MULTI_MAX_READ:
            raise ValueError("max_read exceeds FWS_MSG_MULTI_MAX_READ - 138")
        self.slot = (max_read + _lib.FWS_MSG_FLOW_MAX_PENDING + 15) & ~15
        # the shortest frame: a server's reads hold masked frames (6 bytes), a client's unmasked ones (2)
        self.cap = min(self.slot // (2 if role == "client" else 6) + 1, _lib.FWS_MSG_MULTI_MAX_FRAMES)
        self.msg_cap = self.cap + 1                   # a lead that completes a message, then one per frame
        self.dev = torch.device(device)
        u8 = dict(dtype=torch.uint8, device=self.dev)
        pin = dict(dtype=torch.uint8, pin_memory=True)
        self._sizes = dict(wire=self.slot, dst=self.slot, ctl=self.slot, frames=self.cap * FRAME_INFO.itemsize,
                           msgs=self.msg_cap * MSG_INFO.itemsize, res=DECODE_RESULT.itemsize,
                           mres=MSG_RESULT.itemsize, reads=MSG_READ.itemsize)
        self._d = {k: torch.zeros(n_conns * sz, **u8) for k, sz in self._sizes.items()}
        self._h = {k: torch.zeros(n_conns * sz, **pin) for k, sz in self._sizes.items()}
        self.flows = torch.zeros(n_conns * _lib.MSG_FLOW.itemsize, **u8)
        self._pending = [b""] * n_conns
        self._parts = [[] for _ in range(n_conns)]
        self.status = [0] * n_conns
        self.calls = 0                                # fws_gpu_decode_messages_flow calls made
        self.uploaded = [0] * n_conns                 # wire bytes copied to the device, per connection
        # MessageResponder's hooks: _queued(conns, max_len, stream) right after a call's launch, before its
        # synchronisation; _synced(conns) right after it
        self._queued = self._synced = None

    def _call(self, bufs):
        """One launch for {conn: bytes}: the units per connection; pending, parts and status updated."""
        conns, n = list(bufs), len(bufs)
        sz, hw = self._sizes, self._h["wire"].numpy()
        desc = np.zeros(n, dtype=MSG_READ)
        for i, c in enumerate(conns):
            buf = bufs[c]
            hw[i * self.slot:i * self.slot + len(buf)] = np.frombuffer(buf, dtype=np.uint8)
            desc[i] = (i * self.slot, i * self.slot, i * self.slot, len(buf), c, self.slot, self.slot,
                       i * self.cap, self.cap, i * self.msg_cap, self.msg_cap, 0)
            self.uploaded[c] += len(buf)
        self._h["reads"].numpy()[:n * sz["reads"]] = desc.view(np.uint8)
        stream = torch.cuda.current_stream(self.dev)
        for k in ("wire", "reads"):
            self._d[k][:n * sz[k]].copy_(self._h[k][:n * sz[k]], non_blocking=True)
        max_len = max(1, max(map(len, bufs.values())))
        d = self._d
        check(self._decode_name,
              self._decode(self.ctx, d["wire"], d["reads"], n, max_len, d["frames"], d["msgs"], d["dst"],
                           d["ctl"], d["res"], d["mres"], self.flows, self.n_conns, stream=stream))
        self.calls += 1
        if self._queued:
            self._queued(conns, max_len, stream)
        for k in ("mres", "msgs", "dst", "ctl"):
            self._h[k][:n * sz[k]].copy_(d[k][:n * sz[k]], non_blocking=True)
        stream.synchronize()
        if self._synced:
            self._synced(conns)
        mres = np.frombuffer(self._h["mres"].numpy()[:n * sz["mres"]].tobytes(), dtype=MSG_RESULT)
        out = {}
        for i, c in enumerate(conns):
            r, buf = mres[i], bufs[c]
            status = int(r["status"])
            if status in (_lib.FWS_ERR_DECLINED, _lib.FWS_ERR_INVALID):
                raise FwsError(f"{self._decode_name} refused the read of connection {c}", status)
            entries = np.frombuffer(self._h["msgs"].numpy()[i * sz["msgs"]:i * sz["msgs"] + int(r["n_msgs"]) *
                                                            MSG_INFO.itemsize].tobytes(), dtype=MSG_INFO)
            dst = self._h["dst"].numpy()[i * self.slot:(i + 1) * self.slot]
            ctl = self._h["ctl"].numpy()[i * self.slot:(i + 1) * self.slot]
            units = []
            for e in entries:
                off, ln = int(e["off"]), int(e["len"])
                if e["opcode"] >= 8:
                    units.append((int(e["opcode"]), ctl[off:off + ln].tobytes(), False))
                    continue
                body = dst[off:off + ln].tobytes()
                if e["flags"] & _lib.FWS_MSG_CONTINUED:
                    body = b"".join(self._parts[c]) + body
                self._parts[c] = []
                units.append((int(e["opcode"]), body, bool(e["utf8_ok"])))
            if int(r["open_opcode"]) and int(r["open_len"]):
                off = int(r["open_off"])
                self._parts[c].append(dst[off:off + int(r["open_len"])].tobytes())
            self._pending[c] = buf[int(r["resume_off"]):]
            self.status[c] = status
            out[c] = (units, int(r["resume_off"]))
        return out

    def feed(self, reads):
        for conn, data in reads.items():
            if not 0 <= conn < self.n_conns:
                raise ValueError(f"connection {conn} out of range")
            if self.status[conn] not in (0, _lib.FWS_ERR_CAPACITY):
                raise FwsError(f"MessageFlow.feed after an error on connection {conn}", self.status[conn])
            if len(data) > self.max_read:
                raise ValueError(f"a read of {len(data)} bytes exceeds max_read = {self.max_read}")
        bufs = {c: self._pending[c] + bytes(reads[c]) for c in reads}
        out = {c: [] for c in reads}
        while bufs:
            again = {}
            for c, (units, resume) in self._call(bufs).items():
                out[c] += units
                # more headers than one call takes: the rest of the same bytes, from resume_off
                if self.status[c] == _lib.FWS_ERR_CAPACITY and resume > 0 and self._pending[c]:
                    again[c] = self._pending[c]
            bufs = again
        return out


class DecodeEngine:
    """fws_decode_engine: fws_gpu_decode_stream over many independent streams,
    decodes kept in flight on two HIP streams. mode / scan_cus select the
    schedule through the library's tuning hooks (0: whole decodes alternating
    over the two streams, the default; 1: scans on one stream, resolve + unmask
    on the other, CU-partitioned when scan_cus > 0) -- for A/B runs only."""

    def __init__(self, device=0, max_frames=0, max_stream_bytes=0, mode=None, scan_cus=0):
        L = lib()
        old = None
        if mode is not None:
            old = (L.fws_internal_set_engine_mode(mode), L.fws_internal_set_engine_scan_cus(scan_cus))
        try:
            h = C.c_void_p()
            check("fws_decode_engine_create", L.fws_decode_engine_create(device, max_frames, max_stream_bytes,
                                                                         C.byref(h)))
        finally:
            if old is not None:
                L.fws_internal_set_engine_mode(old[0])
                L.fws_internal_set_engine_scan_cus(old[1])
        self.h = h

    def run(self, jobs, stream=None):
        """jobs: (wire, cap, frames, result[, utf8_ok]) tuples of device tensors
        (len = wire.numel()). Returns the status; nothing synchronised."""
        a = np.zeros(len(jobs), dtype=DECODE_JOB)
        for i, j in enumerate(jobs):
            wire, cap, frames, result = j[:4]
            u = j[4] if len(j) > 4 else None
            a[i] = (wire.data_ptr(), wire.numel(), frames.data_ptr(), cap, 0, result.data_ptr(),
                    u.data_ptr() if u is not None else 0)
        self._jobs = a                                   # alive until the next run
        return lib().fws_decode_engine_run(self.h, C.c_void_p(a.ctypes.data), len(jobs), _stream_handle(stream))

    def close(self):
        if self.h:
            lib().fws_decode_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def read_result(result):
    return np.frombuffer(result.cpu().numpy().tobytes(), dtype=DECODE_RESULT)[0]


def read_frames(frames, count):
    raw = frames[:count * FRAME_INFO.itemsize].cpu().numpy()
    return np.frombuffer(raw.tobytes(), dtype=FRAME_INFO).copy()


def validate_utf8(ctx, base, dev_descs, n, ok, stream=None):
    check("fws_gpu_validate_utf8", lib().fws_gpu_validate_utf8(ctx.h, _ptr(base), _ptr(dev_descs), n,
                                                               _ptr(ok), _stream_handle(stream)))


# ------------------------------------------------------------ workloads
GEN_FIXED, GEN_MIXED, GEN_FRAGMENTED, GEN_UTF8 = 0, 1, 2, 3


def gen_batch(kind, seed=42, opcode=2, n_frames=0, payload_min=0, payload_max=0, target_bytes=0,
              invalid_permille=0):
    """Synthetic client-masked frames (fws_gen_batch). Returns (wire uint8
    numpy array, FRAME_DESC array of payload regions, utf8_ok uint8 array)."""
    p = GenParams(seed=seed, kind=kind, opcode=opcode, n_frames=n_frames, payload_min=payload_min,
                  payload_max=payload_max, target_bytes=target_bytes,
                  invalid_permille=invalid_permille)
    wl, nf = C.c_uint64(0), C.c_uint64(0)
    check("fws_gen_batch", lib().fws_gen_batch(C.byref(p), None, 0, C.byref(wl), None, 0, C.byref(nf),
                                               None))
    wire = np.empty(wl.value, dtype=np.uint8)
    descs = np.zeros(nf.value, dtype=FRAME_DESC)
    ok = np.zeros(nf.value, dtype=np.uint8)
    check("fws_gen_batch", lib().fws_gen_batch(C.byref(p), wire.ctypes.data, wl.value, C.byref(wl),
                                               descs.ctypes.data, nf.value, C.byref(nf), ok.ctypes.data))
    return wire, descs, ok


# BASELINE.json configs as generator calls
def config_c2(seed=42, n_frames=65536, payload=4096):
    return gen_batch(GEN_FIXED, seed=seed, opcode=2, n_frames=n_frames, payload_min=payload)


def config_c3(seed=42, target=256 << 20):
    return gen_batch(GEN_MIXED, seed=seed, opcode=2, payload_min=64, payload_max=65536,
                     target_bytes=target)


def config_c4(seed=42, target=256 << 20):
    return gen_batch(GEN_FRAGMENTED, seed=seed, opcode=2, payload_min=4096, payload_max=1 << 20,
                     target_bytes=target)


def config_c5(seed=42, n_frames=262144, payload=16384, invalid_permille=10):
    return gen_batch(GEN_UTF8, seed=seed, n_frames=n_frames, payload_min=payload,
                     invalid_permille=invalid_permille)


# ------------------------------------------------------------ RX session
class HostArena:
    """Page-aligned host memory registered with fws_gpu_host_register: reads
    placed in it are decoded in place by RxSession / RxMux (the drop-in hook
    registers the reference's MemPool read buffers the same way)."""

    def __init__(self, nbytes):
        self.raw = np.zeros(nbytes + 8192, dtype=np.uint8)
        off = (-self.raw.ctypes.data) % 4096
        self.mem = self.raw[off:off + nbytes]
        check("fws_gpu_host_register", lib().fws_gpu_host_register(self.mem.ctypes.data, nbytes))
        self.pos = 0

    def place(self, data, align_off=0):
        """A view of the arena holding `data`, starting align_off bytes past a
        64-B boundary (the arena is reused round-robin)."""
        n = len(data)
        start = ((self.pos + 63) // 64) * 64 + align_off
        if start + n + 64 > len(self.mem):
            start = align_off
        v = self.mem[start:start + n]
        v[:] = np.frombuffer(bytes(data), dtype=np.uint8)
        self.pos = start + n
        return v

    def close(self):
        if self.mem is not None:
            lib().fws_gpu_host_unregister(self.mem.ctypes.data)
            self.mem = None


class RxSession:
    """fws_rx_session: OnRecvData (w_socket.h:543-769) over the GPU for host reads."""

    def __init__(self, ctx, is_server=True):
        h = C.c_void_p()
        check("fws_rx_session_create", lib().fws_rx_session_create(ctx.h, 1 if is_server else 0, C.byref(h)))
        self.h = h

    def feed(self, data, extra_cap=0, ev_cap=1 << 16, ctl_cap=1 << 20, arena=None, align_off=0):
        """arena: a HostArena to place the read in (decoded in place), else a fresh host copy."""
        buf = (arena.place(data, align_off) if arena is not None
               else np.frombuffer(bytes(data), dtype=np.uint8).copy())
        ev = np.zeros(ev_cap, dtype=RX_EVENT)
        ctl = np.zeros(ctl_cap, dtype=np.uint8)
        n_ev, ctl_used = C.c_uint64(0), C.c_uint64(0)
        ret = lib().fws_rx_session_feed(self.h, buf.ctypes.data if len(buf) else None, len(buf),
                                        len(buf) + extra_cap, ev.ctypes.data, ev_cap, C.byref(n_ev),
                                        ctl.ctypes.data, ctl_cap, C.byref(ctl_used))
        return ret, (buf.copy() if arena is not None else buf), ev[:n_ev.value].copy(), ctl[:ctl_used.value].copy()

    def state(self):
        st = _lib.RxState()
        check("fws_rx_session_state", lib().fws_rx_session_state(self.h, C.byref(st)))
        return st

    def close(self):
        if self.h:
            lib().fws_rx_session_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def check_sorted(ctx, dd, n, stream=None):
    """fws_gpu_check_sorted: the first descriptor index breaking the sorted /
    disjoint contract of unmask_sorted, or None (synchronises)."""
    bad = torch.empty(1, dtype=torch.int32, device=dd.device)
    st = stream if stream is not None else torch.cuda.current_stream()
    check("fws_gpu_check_sorted", lib().fws_gpu_check_sorted(ctx.h, dd.data_ptr(), n, bad.data_ptr(), st.cuda_stream))
    v = int(bad.item()) & 0xFFFFFFFF
    return None if v == 0xFFFFFFFF else v


class RxMux:
    """fws_rx_mux: the reads of many connections decoded in one round trip
    (FLoop::OneStep's shape, floop.h:661-703), each with its own carried state;
    per read the results equal RxSession.feed on that connection alone."""

    def __init__(self, ctx, n_conns):
        h = C.c_void_p()
        check("fws_rx_mux_create", lib().fws_rx_mux_create(ctx.h, n_conns, C.byref(h)))
        self.h = h
        self.n = n_conns

    def feed(self, reads, extra_cap=0, arena=None, align_off=None, between=None):
        """reads: [(conn, bytes)]. Returns [(ret, unmasked bytes, events, ctl bytes)].
        arena: a HostArena the reads are placed in (align_off(i) -> offset past a
        64-B boundary for read i), else fresh host copies. between: a callable run
        while the batch decodes (fws_rx_mux_submit, between(), fws_rx_mux_complete)
        instead of one fws_rx_mux_feed."""
        bufs = [arena.place(d, align_off(i) if align_off else 0) if arena is not None
                else np.frombuffer(bytes(d), dtype=np.uint8).copy() for i, (_, d) in enumerate(reads)]
        rr = np.zeros(len(reads), dtype=_lib.RX_READ)
        for i, ((conn, _), b) in enumerate(zip(reads, bufs)):
            rr[i] = (conn, 0, b.ctypes.data if len(b) else 0, len(b), len(b) + extra_cap)
        out = np.zeros(len(reads), dtype=_lib.RX_READ_RESULT)
        if between is None:
            check("fws_rx_mux_feed", lib().fws_rx_mux_feed(self.h, rr.ctypes.data if len(reads) else None,
                                                           len(reads), out.ctypes.data if len(reads) else None))
        else:
            check("fws_rx_mux_submit", lib().fws_rx_mux_submit(self.h, rr.ctypes.data if len(reads) else None,
                                                               len(reads)))
            between()
            check("fws_rx_mux_complete", lib().fws_rx_mux_complete(self.h, out.ctypes.data if len(reads) else None))
        res = []
        for i, b in enumerate(bufs):
            o = out[i]
            n_ev, n_ctl = int(o["n_events"]), int(o["ctl_used"])
            ev = np.zeros(n_ev, dtype=RX_EVENT)
            if n_ev:
                C.memmove(ev.ctypes.data, int(o["events"]), n_ev * RX_EVENT.itemsize)
            ctl = np.zeros(n_ctl, dtype=np.uint8)
            if n_ctl:
                C.memmove(ctl.ctypes.data, int(o["ctl"]), n_ctl)
            res.append((int(o["ret"]), b.copy() if arena is not None else b, ev, ctl))
        return res

    def submit_raw(self, rr, n):
        """fws_rx_mux_submit on a prepared RX_READ array (tests); returns the code"""
        return int(lib().fws_rx_mux_submit(self.h, rr.ctypes.data if n else None, n))

    def complete_raw(self, out):
        """fws_rx_mux_complete into a prepared RX_READ_RESULT array (tests); returns the code"""
        return int(lib().fws_rx_mux_complete(self.h, out.ctypes.data if len(out) else None))

    def reset(self, conn):
        check("fws_rx_mux_reset", lib().fws_rx_mux_reset(self.h, conn))

    def state(self, conn):
        st = _lib.RxState()
        check("fws_rx_mux_state", lib().fws_rx_mux_state(self.h, conn, C.byref(st)))
        return st

    def close(self):
        if self.h:
            lib().fws_rx_mux_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TxSession:
    """fws_tx_session: SendFrame (w_socket.h:832-944) for host payloads of one
    connection; the frame bytes are built on the GPU."""

    def __init__(self, ctx, is_server=False):
        h = C.c_void_p()
        check("fws_tx_session_create", lib().fws_tx_session_create(ctx.h, 1 if is_server else 0, C.byref(h)))
        self.h = h

    def send(self, frames, out_cap=None):
        """frames: [(payload bytes, frame_type, last, key)]. Returns (rc, wire
        bytes, needed length); rc != 0 leaves the session state unchanged."""
        n = len(frames)
        bufs = [np.frombuffer(bytes(p), dtype=np.uint8).copy() for p, _, _, _ in frames]
        ptrs = np.array([b.ctypes.data if len(b) else 0 for b in bufs], dtype=np.uint64)
        lens = np.array([len(b) for b in bufs], dtype=np.uint64)
        types = np.array([f[1] for f in frames], dtype=np.uint32)
        last = np.array([1 if f[2] else 0 for f in frames], dtype=np.uint8)
        keys = np.array([f[3] & 0xFFFFFFFF for f in frames], dtype=np.uint32)
        cap = int(lens.sum()) + 14 * n if out_cap is None else out_cap
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        ol = C.c_uint64(0)
        rc = lib().fws_tx_session_send(self.h, ptrs.ctypes.data, lens.ctypes.data, types.ctypes.data,
                                       last.ctypes.data, keys.ctypes.data, n, out.ctypes.data, cap, C.byref(ol))
        return rc, out[:ol.value].tobytes() if rc == 0 else b"", ol.value

    def last_msg_not_fin(self):
        v = C.c_uint8(0)
        check("fws_tx_session_state", lib().fws_tx_session_state(self.h, C.byref(v)))
        return v.value

    def close(self):
        if self.h:
            lib().fws_tx_session_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def plan_mode(ctx):
    """The last descriptor plan's mode (diagnostic; synchronises): dict with
    byte_space (payloads sorted and disjoint: byte-space unmask), s0, first_po,
    last_pe, n_units."""
    out = (C.c_uint64 * 5)()
    check("fws_internal_plan_mode", lib().fws_internal_plan_mode(ctx.h, out))
    return dict(zip(("byte_space", "s0", "first_po", "last_pe", "n_units"), list(out)))


def decode_counters(ctx):
    """The last decode's counters on ctx (decode_common.h Counter; diagnostic,
    synchronises): survivors, frames, big-ST super tiles, failure flag."""
    out = (C.c_uint32 * 16)()
    check("fws_internal_decode_counters", lib().fws_internal_decode_counters(ctx.h, out, 16))
    return {"survivors": out[0], "frames": out[3], "failed": out[9] != 0, "big_super_tiles": out[12]}


class RxPipe:
    """fws_rx_pipe: batched, pipelined decode of host batches (H2D -> parse +
    unmask -> D2H on `depth` streams). Batches are pinned CPU uint8 tensors;
    each is unmasked in place once its wait() returns."""

    def __init__(self, device=0, max_batch_bytes=1 << 28, max_frames=1 << 17, depth=3, utf8=False):
        h = C.c_void_p()
        check("fws_rx_pipe_create", lib().fws_rx_pipe_create(device, max_batch_bytes, max_frames, depth,
                                                             1 if utf8 else 0, C.byref(h)))
        self.h = h
        self.max_frames = max_frames
        self.utf8 = utf8

    def submit(self, batch, n=None):
        t = C.c_uint64()
        n = batch.numel() if n is None else n
        check("fws_rx_pipe_submit", lib().fws_rx_pipe_submit(self.h, C.c_void_p(batch.data_ptr()), n, C.byref(t)))
        return t.value

    def wait(self, ticket, copy_frames=True):
        """(frames structured array, result record, utf8 flags or None)."""
        fp, up = C.c_void_p(), C.c_void_p()
        nf = C.c_uint64()
        res = np.zeros(1, dtype=DECODE_RESULT)
        check("fws_rx_pipe_wait", lib().fws_rx_pipe_wait(self.h, ticket, C.byref(fp), C.byref(nf),
                                                         C.c_void_p(res.ctypes.data), C.byref(up)))
        frames = None
        if copy_frames and nf.value:
            raw = (C.c_uint8 * (nf.value * FRAME_INFO.itemsize)).from_address(fp.value)
            frames = np.frombuffer(bytes(raw), dtype=FRAME_INFO)
        ok = None
        if self.utf8 and nf.value:
            ok = np.frombuffer(bytes((C.c_uint8 * nf.value).from_address(up.value)), dtype=np.uint8)
        return frames, res[0], ok

    def close(self):
        if self.h:
            lib().fws_rx_pipe_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def encode_frames(ctx, out, src, dev_descs, n, out_len=None, stream=None):
    """fws_gpu_encode_frames: out (device uint8, 16-B aligned) = the frames of
    dev_descs (device TX_DESC bytes) back to back. Returns the device u64 total
    tensor (~0 if out is too small); nothing synchronised."""
    if out_len is None:
        out_len = torch.empty(1, dtype=torch.int64, device=out.device)
    check("fws_gpu_encode_frames", lib().fws_gpu_encode_frames(ctx.h, _ptr(out), out.numel(), _ptr(src),
                                                               _ptr(dev_descs), n, _ptr(out_len),
                                                               _stream_handle(stream)))
    return out_len


class TxState:
    """One connection's send sequencing (fws_tx_next, SendFrame's opcode / FIN rule)."""

    def __init__(self):
        self.last_msg_not_fin = C.c_uint8(0)

    def next(self, frame_type, last):
        op, fin = C.c_uint8(), C.c_uint8()
        lib().fws_tx_next(frame_type, int(last), C.byref(self.last_msg_not_fin), C.byref(op), C.byref(fin))
        return op.value, fin.value


def encode_messages_multi(ctx, out, src, sends, n, max_len, frames, results, conns, n_conns, stream=None):
    """fws_gpu_encode_messages_multi: the sends of many connections cut into
    frames and encoded in one launch. sends holds n fws_tx_send descriptors
    (_lib.TX_SEND) in a device uint8 tensor, results n fws_tx_result
    (_lib.TX_RESULT), conns n_conns fws_tx_conn states (_lib.TX_CONN, zeros for
    new connections); frames (FRAME_INFO records) may be None when every
    frame_cap is 0. Returns the call's status; nothing is synchronised."""
    return lib().fws_gpu_encode_messages_multi(ctx.h, _ptr(out), _ptr(src), _ptr(sends), n, max_len,
                                               _ptr(frames) if frames is not None else None, _ptr(results),
                                               _ptr(conns), n_conns, _stream_handle(stream))


def read_tx_conn(conns, conn=0):
    sz = _lib.TX_CONN.itemsize
    return np.frombuffer(conns[conn * sz:(conn + 1) * sz].cpu().numpy().tobytes(), dtype=_lib.TX_CONN)[0]


class MessageSender:
    """The send side of MessageFlow: send({conn: (frame_type, payload, last)})
    makes one upload, one fws_gpu_encode_messages_multi call and one
    synchronisation for all connections and returns {conn: wire bytes}. The
    opcode / FIN sequencing state of every connection stays on the device
    (self.conns). A payload over max_send is cut into pieces that are multiples
    of max_frame and sent by successive calls inside the same send (each one
    upload, one launch, one synchronisation), `last` on the final piece only;
    piece i of a masked message starts its keys where piece i - 1 stopped
    (FWS_TX_FRAG_KEY(key, frames before it)), so frame f of the message has
    FWS_TX_FRAG_KEY(key, f). pieces[conn] = [(offset, length, key), ...] of the
    last send; calls counts the launches."""

    def __init__(self, ctx, n_conns, max_send, device="cuda:0"):
        if not 1 <= max_send <= _lib.FWS_TX_MULTI_MAX_SEND:
            raise ValueError("max_send must be 1..FWS_TX_MULTI_MAX_SEND")
        self.ctx, self.n_conns, self.max_send = ctx, n_conns, max_send
        self.src_slot = (max_send + 15) & ~15
        self.out_slot = (max_send + 14 * _lib.FWS_TX_MULTI_MAX_FRAMES + 15) & ~15
        self.dev = torch.device(device)
        u8 = dict(dtype=torch.uint8, device=self.dev)
        pin = dict(dtype=torch.uint8, pin_memory=True)
        self._sizes = dict(src=self.src_slot, out=self.out_slot, sends=_lib.TX_SEND.itemsize,
                           res=_lib.TX_RESULT.itemsize)
        self._d = {k: torch.zeros(n_conns * sz, **u8) for k, sz in self._sizes.items()}
        self._h = {k: torch.zeros(n_conns * sz, **pin) for k, sz in self._sizes.items()}
        self.conns = torch.zeros(n_conns * _lib.TX_CONN.itemsize, **u8)
        self.calls = 0
        self.pieces = {}

    def _call(self, work, max_frame, masked):
        """One launch for {conn: (frame_type, piece, last, key)}: the wire bytes per connection."""
        conns, n = list(work), len(work)
        sz, hs = self._sizes, self._h["src"].numpy()
        desc = np.zeros(n, dtype=_lib.TX_SEND)
        for i, c in enumerate(conns):
            ft, piece, last, key = work[c]
            hs[i * self.src_slot:i * self.src_slot + len(piece)] = np.frombuffer(piece, dtype=np.uint8)
            d = desc[i]
            d["src_off"], d["out_off"], d["len"], d["out_cap"] = i * self.src_slot, i * self.out_slot, len(piece), \
                self.out_slot
            d["conn"], d["max_frame"], d["key"], d["frame_type"] = c, max_frame, key, ft
            d["last"], d["masked"] = int(bool(last)), int(bool(masked))
        self._h["sends"].numpy()[:n * sz["sends"]] = desc.view(np.uint8)
        stream = torch.cuda.current_stream(self.dev)
        for k in ("src", "sends"):
            self._d[k][:n * sz[k]].copy_(self._h[k][:n * sz[k]], non_blocking=True)
        max_len = max(1, max(len(w[1]) for w in work.values()))
        d = self._d
        check("fws_gpu_encode_messages_multi",
              encode_messages_multi(self.ctx, d["out"], d["src"], d["sends"], n, max_len, None, d["res"], self.conns,
                                    self.n_conns, stream=stream))
        self.calls += 1
        for k in ("res", "out"):
            self._h[k][:n * sz[k]].copy_(d[k][:n * sz[k]], non_blocking=True)
        stream.synchronize()
        res = np.frombuffer(self._h["res"].numpy()[:n * sz["res"]].tobytes(), dtype=_lib.TX_RESULT)
        out = {}
        for i, c in enumerate(conns):
            if int(res[i]["status"]):
                raise FwsError(f"fws_gpu_encode_messages_multi refused the send of connection {c}",
                               int(res[i]["status"]))
            o = i * self.out_slot
            out[c] = self._h["out"].numpy()[o:o + int(res[i]["out_len"])].tobytes()
        return out

    def send(self, sends, max_frame=0, keys=None, masked=True):
        step = self.max_send
        if max_frame:
            step = min(self.max_send // max_frame, _lib.FWS_TX_MULTI_MAX_FRAMES) * max_frame
        queue, self.pieces = {}, {}
        for conn, (ft, payload, last) in sends.items():
            if not 0 <= conn < self.n_conns:
                raise ValueError(f"connection {conn} out of range")
            payload = bytes(payload)
            if keys is not None:
                key = keys[conn] & 0xFFFFFFFF
            else:
                key = int(np.random.randint(0, 1 << 32, dtype=np.uint64)) if masked else 0
            control = bool(ft & 8)
            if control or len(payload) <= (step if max_frame else self.max_send):
                cuts = [(0, len(payload))]
            elif not max_frame or step == 0:
                raise ValueError(f"a send of {len(payload)} bytes exceeds max_send = {self.max_send} and "
                                 f"max_frame = {max_frame} gives no piece size")
            else:
                cuts = [(o, min(step, len(payload) - o)) for o in range(0, len(payload), step)]
            per = step // max_frame if max_frame else 0
            self.pieces[conn] = [(o, ln, _lib.FWS_TX_FRAG_KEY(key, i * per)) for i, (o, ln) in enumerate(cuts)]
            queue[conn] = [(ft, payload[o:o + ln], bool(last) and i + 1 == len(cuts), k)
                           for i, (o, ln, k) in enumerate(self.pieces[conn])]
        out = {c: b"" for c in sends}
        while queue:
            work = {c: q.pop(0) for c, q in queue.items()}
            for c, b in self._call(work, max_frame, masked).items():
                out[c] += b
            queue = {c: q for c, q in queue.items() if q}
        return out


def reply_messages_multi(ctx, reads, n, max_len, msgs, dst, ctl, msg_results, regions, out, frames, results, conns,
                         states, n_conns, flags, stream=None):
    """fws_gpu_reply_messages_multi: the reply frames of n decoded reads in one
    launch. reads, msgs, dst, ctl and msg_results are the tensors the decode
    call (decode_messages_flow / decode_messages_multi) was given, max_len its
    value; regions holds n fws_reply_region (_lib.REPLY_REGION), results n
    fws_tx_result, conns n_conns fws_tx_conn (the array encode_messages_multi
    takes), states n_conns fws_reply_state (_lib.REPLY_STATE, zeros for new
    connections); frames may be None when every frame_cap is 0. flags:
    _lib.FWS_REPLY_CONTROL | _lib.FWS_REPLY_ECHO. Returns the call's status;
    nothing is synchronised."""
    return lib().fws_gpu_reply_messages_multi(ctx.h, _ptr(reads), n, max_len, _ptr(msgs), _ptr(dst), _ptr(ctl),
                                              _ptr(msg_results), _ptr(regions), _ptr(out),
                                              _ptr(frames) if frames is not None else None, _ptr(results),
                                              _ptr(conns), _ptr(states), n_conns, flags, _stream_handle(stream))


def reply_messages_strict(ctx, reads, n, max_len, msgs, dst, ctl, msg_results, conn_states, conn_state_stride,
                          max_message_bytes, regions, out, frames, results, conns, states, n_conns, flags, stream=None):
    """fws_gpu_reply_messages_strict: reply_messages_multi for a server that
    fails connections on the device. conn_states is the decode call's own state
    tensor (fws_msg_carry records, conn_state_stride 64, after
    decode_messages_multi; fws_msg_flow records, 96, after decode_messages_flow),
    read only; max_message_bytes bounds a message (0: no limit). A read's first
    failing item -- a message over the limit, a TEXT message or CLOSE reason that
    is not UTF-8, a malformed CLOSE, a decode that ended in a protocol error --
    is answered with a CLOSE carrying 1009, 1007 or 1002, nothing follows it and
    fws_reply_state.fail_code keeps the code. Returns the call's status; nothing
    is synchronised."""
    return lib().fws_gpu_reply_messages_strict(ctx.h, _ptr(reads), n, max_len, _ptr(msgs), _ptr(dst), _ptr(ctl),
                                               _ptr(msg_results), _ptr(conn_states), conn_state_stride,
                                               max_message_bytes, _ptr(regions), _ptr(out),
                                               _ptr(frames) if frames is not None else None, _ptr(results),
                                               _ptr(conns), _ptr(states), n_conns, flags, _stream_handle(stream))


def reply_messages_multi_client(ctx, reads, n, max_len, msgs, dst, ctl, msg_results, regions, out, frames, results,
                                conns, states, n_conns, flags, keys, stream=None):
    """fws_gpu_reply_messages_multi_client: reply_messages_multi writing client
    frames -- the MASK bit, 4 key bytes, the payload XORed. keys is a device
    tensor of n uint32 words, one per read; frame j of read r is masked with
    _lib.FWS_TX_FRAG_KEY(keys[r], j). The other arguments are
    reply_messages_multi's, the decode call's tensors those of
    decode_messages_flow_client. Returns the call's status; nothing is
    synchronised."""
    return lib().fws_gpu_reply_messages_multi_client(ctx.h, _ptr(reads), n, max_len, _ptr(msgs), _ptr(dst), _ptr(ctl),
                                                     _ptr(msg_results), _ptr(regions), _ptr(out),
                                                     _ptr(frames) if frames is not None else None, _ptr(results),
                                                     _ptr(conns), _ptr(states), n_conns, flags,
                                                     _ptr(keys) if keys is not None else None,
                                                     _stream_handle(stream))


def reply_messages_strict_client(ctx, reads, n, max_len, msgs, dst, ctl, msg_results, conn_states, conn_state_stride,
                                 max_message_bytes, regions, out, frames, results, conns, states, n_conns, flags,
                                 keys, stream=None):
    """fws_gpu_reply_messages_strict_client: reply_messages_strict writing client
    frames, keys as in reply_messages_multi_client; the failing CLOSE is a masked
    frame of 8 bytes and counts in the key's frame index. Returns the call's
    status; nothing is synchronised."""
    return lib().fws_gpu_reply_messages_strict_client(ctx.h, _ptr(reads), n, max_len, _ptr(msgs), _ptr(dst),
                                                      _ptr(ctl), _ptr(msg_results), _ptr(conn_states),
                                                      conn_state_stride, max_message_bytes, _ptr(regions), _ptr(out),
                                                      _ptr(frames) if frames is not None else None, _ptr(results),
                                                      _ptr(conns), _ptr(states), n_conns, flags,
                                                      _ptr(keys) if keys is not None else None,
                                                      _stream_handle(stream))


def read_reply_state(states, conn=0):
    sz = _lib.REPLY_STATE.itemsize
    return np.frombuffer(states[conn * sz:(conn + 1) * sz].cpu().numpy().tobytes(), dtype=_lib.REPLY_STATE)[0]


class MessageResponder:
    """A MessageFlow that answers on the device: feed({conn: bytes}) returns
    (units, replies), units exactly what flow.feed returns and replies[conn] the
    connection's reply wire bytes -- PONGs and the CLOSE echo with
    FWS_REPLY_CONTROL, every data part as a frame with FWS_REPLY_ECHO --
    concatenated over the decode calls the feed made. Each reply launch is
    queued right behind its decode launch, before that call's one
    synchronisation; the send sequencing (self.conns, which an application's
    encode_messages_multi sends share) and the reply states (self.states) stay
    on the device. With strict=True the launches are
    fws_gpu_reply_messages_strict over flow's state tensor: a connection that
    breaks the protocol, sends a TEXT message or CLOSE reason that is not UTF-8
    or a message over max_message bytes (0: no limit) gets its valid prefix
    answered and then a CLOSE with the status code; failed = {conn: code} lists
    these connections (flow.status[conn] keeps a decode error as before, and
    the host drops the connection). Over a client-role flow
    (MessageFlow(role="client")) the launches are the _client calls and the
    replies are masked: every call uploads one key per read with the
    descriptors, key_fn(conn) -> u32 (random.getrandbits(32) by default), and
    last_keys = {conn: key} keeps the last call's, so frame j of that call's
    reply on conn was masked with _lib.FWS_TX_FRAG_KEY(last_keys[conn], j).
    Over a server-role flow key_fn must be None."""

    def __init__(self, flow, flags, device="cuda:0", strict=False, max_message=0, key_fn=None):
        self.flow, self.flags, self.strict, self.max_message = flow, flags, bool(strict), int(max_message)
        self.client = getattr(flow, "role", "server") == "client"
        if key_fn is not None and not self.client:
            raise ValueError("key_fn is for a client-role flow: a server's replies are not masked")
        self.key_fn = key_fn if key_fn is not None else (lambda conn: random.getrandbits(32))
        self.last_keys = {}
        self.failed = {}
        self.dev = torch.device(device)
        n = flow.n_conns
        # a read's replies: its payload bytes and a header per entry and for the open part
        # (strict: and the 4 bytes of the failing CLOSE; a client: and 4 key bytes per frame)
        hdr = 14 if self.client else 10
        fail = (8 if self.client else 4) if self.strict else 0
        self.out_slot = (flow.slot + hdr * (flow.msg_cap + 1) + fail + 15) & ~15
        u8 = dict(dtype=torch.uint8, device=self.dev)
        pin = dict(dtype=torch.uint8, pin_memory=True)
        self._sizes = dict(out=self.out_slot, res=_lib.TX_RESULT.itemsize, regions=_lib.REPLY_REGION.itemsize,
                           **(dict(keys=4) if self.client else {}))
        self._d = {k: torch.zeros(n * sz, **u8) for k, sz in self._sizes.items()}
        self._h = {k: torch.zeros(n * sz, **pin) for k, sz in self._sizes.items()}
        self.conns = torch.zeros(n * _lib.TX_CONN.itemsize, **u8)
        self.states = torch.zeros(n * _lib.REPLY_STATE.itemsize, **u8)
        self._h_states = torch.zeros(n * _lib.REPLY_STATE.itemsize, **pin)
        regions = np.zeros(n, dtype=_lib.REPLY_REGION)   # slot i is read i's, whichever connection that is
        regions["out_off"] = np.arange(n, dtype=np.uint64) * np.uint64(self.out_slot)
        regions["out_cap"] = self.out_slot
        self._d["regions"].copy_(torch.from_numpy(regions.view(np.uint8).copy()))
        self.calls = 0
        self._replies = None

    def _queued(self, conns, max_len, stream):
        n, d, f, sz = len(conns), self._d, self.flow._d, self._sizes
        if self.client:
            self._queue_client(conns, max_len, stream)
        elif self.strict:
            check("fws_gpu_reply_messages_strict",
                  reply_messages_strict(self.flow.ctx, f["reads"], n, max_len, f["msgs"], f["dst"], f["ctl"], f["mres"],
                                        self.flow.flows, _lib.MSG_FLOW.itemsize, self.max_message, d["regions"],
                                        d["out"], None, d["res"], self.conns, self.states, self.flow.n_conns,
                                        self.flags, stream=stream))
        else:
            check("fws_gpu_reply_messages_multi",
                  reply_messages_multi(self.flow.ctx, f["reads"], n, max_len, f["msgs"], f["dst"], f["ctl"], f["mres"],
                                       d["regions"], d["out"], None, d["res"], self.conns, self.states,
                                       self.flow.n_conns, self.flags, stream=stream))
        self.calls += 1
        for k in ("res", "out"):
            self._h[k][:n * sz[k]].copy_(d[k][:n * sz[k]], non_blocking=True)
        if self.strict:
            self._h_states.copy_(self.states, non_blocking=True)

    def _queue_client(self, conns, max_len, stream):
        """The client form of the launch: the keys go up with it, one per read."""
        n, d, f = len(conns), self._d, self.flow._d
        self.last_keys = {c: int(self.key_fn(c)) & 0xFFFFFFFF for c in conns}
        self._h["keys"].numpy()[:4 * n] = np.array([self.last_keys[c] for c in conns], dtype="<u4").view(np.uint8)
        d["keys"][:4 * n].copy_(self._h["keys"][:4 * n], non_blocking=True)
        if self.strict:
            check("fws_gpu_reply_messages_strict_client",
                  reply_messages_strict_client(self.flow.ctx, f["reads"], n, max_len, f["msgs"], f["dst"], f["ctl"],
                                               f["mres"], self.flow.flows, _lib.MSG_FLOW.itemsize, self.max_message,
                                               d["regions"], d["out"], None, d["res"], self.conns, self.states,
                                               self.flow.n_conns, self.flags, d["keys"], stream=stream))
        else:
            check("fws_gpu_reply_messages_multi_client",
                  reply_messages_multi_client(self.flow.ctx, f["reads"], n, max_len, f["msgs"], f["dst"], f["ctl"],
                                              f["mres"], d["regions"], d["out"], None, d["res"], self.conns,
                                              self.states, self.flow.n_conns, self.flags, d["keys"], stream=stream))

    def _synced(self, conns):
        n = len(conns)
        res = np.frombuffer(self._h["res"].numpy()[:n * self._sizes["res"]].tobytes(), dtype=_lib.TX_RESULT)
        for i, c in enumerate(conns):
            if int(res[i]["status"]):
                raise FwsError(f"fws_gpu_reply_messages_multi refused the read of connection {c}",
                               int(res[i]["status"]))
            o = i * self.out_slot
            self._replies[c] = self._replies.get(c, b"") + self._h["out"].numpy()[o:o + int(res[i]["out_len"])].tobytes()
        if self.strict:
            states = np.frombuffer(self._h_states.numpy().tobytes(), dtype=_lib.REPLY_STATE)
            for c in conns:
                if int(states[c]["fail_code"]):
                    self.failed[c] = int(states[c]["fail_code"])

    def feed(self, reads):
        self._replies = {c: b"" for c in reads}
        self.flow._queued, self.flow._synced = self._queued, self._synced
        try:
            units = self.flow.feed(reads)
        finally:
            self.flow._queued = self.flow._synced = None
        return units, self._replies


def join_messages(ctx, reads, n, max_len, msgs, dst, msg_results, store, store_stride, joined, results, states,
                  n_conns, stream=None):
    """fws_gpu_join_messages: the messages that span reads put together on the
    device. reads, msgs, dst and msg_results are the tensors the decode call
    (decode_messages_flow, _flow_client or decode_messages_multi) was given,
    max_len its value; store holds n_conns slots of store_stride bytes (two
    halves each), joined one fws_join_info (_lib.JOIN_INFO) per decode entry at
    the entry's index, results n fws_join_result (_lib.JOIN_RESULT), states
    n_conns fws_join_state (_lib.JOIN_STATE, zeros for new connections). Returns
    the call's status; nothing is synchronised."""
    return lib().fws_gpu_join_messages(ctx.h, _ptr(reads), n, max_len, _ptr(msgs), _ptr(dst), _ptr(msg_results),
                                       _ptr(store), store_stride, _ptr(joined), _ptr(results), _ptr(states), n_conns,
                                       _stream_handle(stream))


def read_join_state(states, conn=0):
    sz = _lib.JOIN_STATE.itemsize
    return np.frombuffer(states[conn * sz:(conn + 1) * sz].cpu().numpy().tobytes(), dtype=_lib.JOIN_STATE)[0]


class MessageJoiner:
    """A MessageFlow whose messages are joined on the device: feed({conn:
    bytes}) returns what flow.feed returns, but every data message's bytes are
    read from where its fws_join_info record points -- the read's region of dst,
    or, for a message that arrived over several reads, the connection's slot of
    self.store (2 * align16(max_message) bytes, two halves), where a consumer on
    the device finds it whole until the connection's next call. The join launch
    is queued right behind each decode launch, the retries on the header limit
    included; the join states (self.states) stay on the device, the host keeps
    no parts (flow._parts is not used) and copies back from the store only the
    messages delivered there. A message of more than align16(max_message) bytes
    is dropped and returned as (opcode, None, utf8_ok).
    A MessageJoiner stands in for its flow: MessageResponder(joiner, flags, ...)
    answers on the device what the joiner decodes. The responder's hooks go on
    the joiner, which calls them -- and any the flow itself carries -- around
    its own launch; they are chained, not replaced."""

    def __init__(self, flow, max_message, device="cuda:0"):
        self.flow, self.max_message = flow, int(max_message)
        self.half = max(16, (self.max_message + 15) & ~15)
        self.stride = 2 * self.half
        self.dev = torch.device(device)
        n = flow.n_conns
        u8 = dict(dtype=torch.uint8, device=self.dev)
        pin = dict(dtype=torch.uint8, pin_memory=True)
        self._jsizes = dict(joined=flow.msg_cap * _lib.JOIN_INFO.itemsize, jres=_lib.JOIN_RESULT.itemsize)
        self._jd = {k: torch.zeros(n * sz, **u8) for k, sz in self._jsizes.items()}
        self._jh = {k: torch.zeros(n * sz, **pin) for k, sz in self._jsizes.items()}
        self.store = torch.zeros(n * self.stride, **u8)
        self._h_store = torch.zeros(n * self.half, **pin)
        self.states = torch.zeros(n * _lib.JOIN_STATE.itemsize, **u8)
        self.calls = 0                                # fws_gpu_join_messages calls made
        self.store_copies = 0                         # messages copied back from the store
        self._queued = self._synced = None            # a MessageResponder's hooks, as on a MessageFlow

    def __getattr__(self, name):                      # what a MessageResponder asks of its flow
        if name == "flow":
            raise AttributeError(name)
        return getattr(self.flow, name)

    def _call(self, bufs):
        """MessageFlow._call with the join launch behind the decode launch: the units per connection."""
        f = self.flow
        conns, n = list(bufs), len(bufs)
        sz, hw = f._sizes, f._h["wire"].numpy()
        desc = np.zeros(n, dtype=MSG_READ)
        for i, c in enumerate(conns):
            buf = bufs[c]
            hw[i * f.slot:i * f.slot + len(buf)] = np.frombuffer(buf, dtype=np.uint8)
            desc[i] = (i * f.slot, i * f.slot, i * f.slot, len(buf), c, f.slot, f.slot, i * f.cap, f.cap,
                       i * f.msg_cap, f.msg_cap, 0)
            f.uploaded[c] += len(buf)
        f._h["reads"].numpy()[:n * sz["reads"]] = desc.view(np.uint8)
        stream = torch.cuda.current_stream(f.dev)
        for k in ("wire", "reads"):
            f._d[k][:n * sz[k]].copy_(f._h[k][:n * sz[k]], non_blocking=True)
        max_len = max(1, max(map(len, bufs.values())))
        d = f._d
        check(f._decode_name,
              f._decode(f.ctx, d["wire"], d["reads"], n, max_len, d["frames"], d["msgs"], d["dst"], d["ctl"],
                        d["res"], d["mres"], f.flows, f.n_conns, stream=stream))
        f.calls += 1
        check("fws_gpu_join_messages",
              join_messages(f.ctx, d["reads"], n, max_len, d["msgs"], d["dst"], d["mres"], self.store, self.stride,
                            self._jd["joined"], self._jd["jres"], self.states, f.n_conns, stream=stream))
        self.calls += 1
        for hook in (f._queued, self._queued):
            if hook:
                hook(conns, max_len, stream)
        for k in ("mres", "dst", "ctl"):
            f._h[k][:n * sz[k]].copy_(d[k][:n * sz[k]], non_blocking=True)
        for k, s in self._jsizes.items():
            self._jh[k][:n * s].copy_(self._jd[k][:n * s], non_blocking=True)
        stream.synchronize()
        for hook in (f._synced, self._synced):
            if hook:
                hook(conns)
        mres = np.frombuffer(f._h["mres"].numpy()[:n * sz["mres"]].tobytes(), dtype=MSG_RESULT)
        jres = np.frombuffer(self._jh["jres"].numpy()[:n * self._jsizes["jres"]].tobytes(), dtype=_lib.JOIN_RESULT)
        recs, stored = [], []
        for i, c in enumerate(conns):
            status = int(mres[i]["status"])
            if status in (_lib.FWS_ERR_DECLINED, _lib.FWS_ERR_INVALID):
                raise FwsError(f"{f._decode_name} refused the read of connection {c}", status)
            if int(jres[i]["status"]):
                raise FwsError(f"fws_gpu_join_messages refused the read of connection {c}", int(jres[i]["status"]))
            o = i * self._jsizes["joined"]
            r = np.frombuffer(self._jh["joined"].numpy()[o:o + int(jres[i]["n_joined"]) *
                                                        _lib.JOIN_INFO.itemsize].tobytes(), dtype=_lib.JOIN_INFO)
            recs.append(r)
            stored += [(int(e["off"]), int(e["len"])) for e in r if e["where"] == _lib.FWS_JOIN_IN_STORE]
        at, back = 0, {}
        for off, ln in stored:                        # (a read delivers one such message at most)
            self._h_store[at:at + ln].copy_(self.store[off:off + ln], non_blocking=True)
            back[off] = at
            at += ln
        if stored:
            stream.synchronize()
            self.store_copies += len(stored)
        hdst, hctl, hst = f._h["dst"].numpy(), f._h["ctl"].numpy(), self._h_store.numpy()
        out = {}
        for i, c in enumerate(conns):
            units = []
            for e in recs[i]:
                off, ln, where = int(e["off"]), int(e["len"]), int(e["where"])
                if where == _lib.FWS_JOIN_IN_CTL:
                    units.append((int(e["opcode"]), hctl[off:off + ln].tobytes(), False))
                elif where == _lib.FWS_JOIN_IN_DST:
                    units.append((int(e["opcode"]), hdst[off:off + ln].tobytes(), bool(e["utf8_ok"])))
                elif where == _lib.FWS_JOIN_IN_STORE:
                    units.append((int(e["opcode"]), hst[back[off]:back[off] + ln].tobytes(), bool(e["utf8_ok"])))
                else:                                 # dropped: longer than a half
                    units.append((int(e["opcode"]), None, bool(e["utf8_ok"])))
            resume = int(mres[i]["resume_off"])
            f._pending[c] = bufs[c][resume:]
            f.status[c] = int(mres[i]["status"])
            out[c] = (units, resume)
        return out

    def feed(self, reads):
        f = self.flow
        for conn, data in reads.items():
            if not 0 <= conn < f.n_conns:
                raise ValueError(f"connection {conn} out of range")
            if f.status[conn] not in (0, _lib.FWS_ERR_CAPACITY):
                raise FwsError(f"MessageJoiner.feed after an error on connection {conn}", f.status[conn])
            if len(data) > f.max_read:
                raise ValueError(f"a read of {len(data)} bytes exceeds max_read = {f.max_read}")
        bufs = {c: f._pending[c] + bytes(reads[c]) for c in reads}
        out = {c: [] for c in reads}
        while bufs:
            again = {}
            for c, (units, resume) in self._call(bufs).items():
                out[c] += units
                # more headers than one call takes: the rest of the same bytes, from resume_off, joined as well
                if f.status[c] == _lib.FWS_ERR_CAPACITY and resume > 0 and f._pending[c]:
                    again[c] = f._pending[c]
            bufs = again
        return out


def publish_messages(ctx, msgs, n_msgs, dst, store, ctl, lst, n_list, subs, n, max_len, out, frames, results, conns,
                     states, n_conns, stream=None):
    """fws_gpu_publish_messages: the listed messages of n subscribers written as
    server frames in one launch. msgs holds n_msgs fws_join_info records
    (_lib.JOIN_INFO: what join_messages wrote, or the application's own), dst /
    store / ctl the buffers their `where` names (None where no record names
    it), lst n_list uint32 indices into msgs, subs n fws_pub_sub
    (_lib.PUB_SUB), results n fws_tx_result, conns n_conns fws_tx_conn (the
    array encode_messages_multi and the reply calls take), states n_conns
    fws_reply_state; frames may be None when every frame_cap is 0. Returns the
    call's status; nothing is synchronised."""
    opt = lambda t: _ptr(t) if t is not None else None   # noqa: E731
    return lib().fws_gpu_publish_messages(ctx.h, _ptr(msgs), n_msgs, opt(dst), opt(store), opt(ctl), _ptr(lst), n_list,
                                          _ptr(subs), n, max_len, _ptr(out), opt(frames), _ptr(results), _ptr(conns),
                                          _ptr(states), n_conns, _stream_handle(stream))


class MessagePublisher:
    """Fan-out for a server: publish(messages, lists) with messages = [(opcode,
    bytes), ...] and lists = {conn: [index, ...]} writes, for every connection
    named, the frames of its listed messages in list order -- one upload (the
    payloads, their records, the lists and the subscribers in one block), one
    fws_gpu_publish_messages call and one synchronisation -- and returns {conn:
    wire bytes}. Equal lists are uploaded once and shared by their subscribers.
    A refused subscriber raises FwsError with its status (the other
    subscribers' frames of that call are written and counted all the same).
    max_out is a connection's region: the most wire bytes one publish may give
    it. conns / states: the fws_tx_conn / fws_reply_state tensors of a
    MessageSender (sender.conns) or MessageResponder to sequence one
    connection's frames through one state; by default the publisher owns zeroed
    ones. calls counts the launches."""

    def __init__(self, ctx, n_conns, max_out, device="cuda:0", conns=None, states=None):
        if max_out < 1:
            raise ValueError("max_out must be at least 1")
        self.ctx, self.n_conns = ctx, n_conns
        self.out_slot = (int(max_out) + 15) & ~15
        self.dev = torch.device(device)
        u8 = dict(dtype=torch.uint8, device=self.dev)
        pin = dict(dtype=torch.uint8, pin_memory=True)
        self._sizes = dict(out=self.out_slot, res=_lib.TX_RESULT.itemsize)
        self._d = {k: torch.zeros(n_conns * sz, **u8) for k, sz in self._sizes.items()}
        self._h = {k: torch.zeros(n_conns * sz, **pin) for k, sz in self._sizes.items()}
        self.conns = conns if conns is not None else torch.zeros(n_conns * _lib.TX_CONN.itemsize, **u8)
        self.states = states if states is not None else torch.zeros(n_conns * _lib.REPLY_STATE.itemsize, **u8)
        self._up_d = self._up_h = None                # the upload block, grown when a publish needs more
        self.calls = 0
        self.lists_uploaded = 0                       # distinct lists of the last publish

    def _block(self, nbytes):
        if self._up_d is None or self._up_d.numel() < nbytes:
            size = max(4096, 1 << (nbytes - 1).bit_length())
            self._up_d = torch.zeros(size, dtype=torch.uint8, device=self.dev)
            self._up_h = torch.zeros(size, dtype=torch.uint8, pin_memory=True)
        return self._up_h.numpy()

    def publish(self, messages, lists):
        conns = list(lists)
        for c in conns:
            if not 0 <= c < self.n_conns:
                raise ValueError(f"connection {c} out of range")
        if not conns:
            return {}
        messages = [(int(op), bytes(p)) for op, p in messages]
        # the block: records | lists | subscribers | payloads, each part 16-B aligned
        recs = np.zeros(len(messages), dtype=_lib.JOIN_INFO)
        at = 0
        for i, (op, p) in enumerate(messages):
            recs[i]["off"], recs[i]["len"], recs[i]["opcode"] = at, len(p), op
            recs[i]["where"], recs[i]["utf8_ok"] = _lib.FWS_JOIN_IN_DST, 1
            at += len(p)
        pay_len = at
        where, flat = {}, []
        for c in conns:
            key = tuple(int(i) for i in lists[c])
            if key not in where:
                where[key] = len(flat)
                flat += key
        self.lists_uploaded = len(where)
        lst = np.asarray(flat, dtype=np.uint32)
        subs = np.zeros(len(conns), dtype=_lib.PUB_SUB)
        for i, c in enumerate(conns):
            key = tuple(int(x) for x in lists[c])
            subs[i] = (i * self.out_slot, self.out_slot, c, where[key], len(key), 0, 0)
        a16 = lambda v: (v + 15) & ~15                # noqa: E731
        o_recs = 0
        o_list = a16(o_recs + recs.nbytes)
        o_subs = a16(o_list + lst.nbytes)
        o_pay = a16(o_subs + subs.nbytes)
        total = o_pay + max(16, pay_len)
        h = self._block(total)
        h[o_recs:o_recs + recs.nbytes] = recs.view(np.uint8)
        h[o_list:o_list + lst.nbytes] = lst.view(np.uint8)
        h[o_subs:o_subs + subs.nbytes] = subs.view(np.uint8)
        at = o_pay
        for _, p in messages:
            h[at:at + len(p)] = np.frombuffer(p, dtype=np.uint8)
            at += len(p)
        stream = torch.cuda.current_stream(self.dev)
        d = self._up_d
        d[:total].copy_(self._up_h[:total], non_blocking=True)
        n, sz = len(conns), self._sizes
        max_len = max([1] + [len(p) for op, p in messages if op in (1, 2)])
        check("fws_gpu_publish_messages",
              publish_messages(self.ctx, d[o_recs:], len(messages), d[o_pay:], None, None, d[o_list:], len(lst),
                               d[o_subs:], n, min(max_len, _lib.FWS_TX_MULTI_MAX_SEND), self._d["out"], None,
                               self._d["res"], self.conns, self.states, self.n_conns, stream=stream))
        self.calls += 1
        for k in ("res", "out"):
            self._h[k][:n * sz[k]].copy_(self._d[k][:n * sz[k]], non_blocking=True)
        stream.synchronize()
        res = np.frombuffer(self._h["res"].numpy()[:n * sz["res"]].tobytes(), dtype=_lib.TX_RESULT)
        out = {}
        for i, c in enumerate(conns):
            if int(res[i]["status"]):
                raise FwsError(f"fws_gpu_publish_messages refused the subscriber of connection {c}",
                               int(res[i]["status"]))
            o = i * self.out_slot
            out[c] = self._h["out"].numpy()[o:o + int(res[i]["out_len"])].tobytes()
        return out
