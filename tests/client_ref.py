"""The client role's predictors and stream builders.

ClientFlowRef is FlowRef (msgflow_ref.py) with the header parse in the client
role: it predicts every output of one fws_gpu_decode_messages_flow_client call.
A MASK bit is FWS_ERR_MASKED, a header is 2, 4 or 10 bytes, the key is 0, so the
walk's unmask copies and frame_key stays 0; nothing else of the walk differs,
which is why FlowRef's own code runs with only its parse exchanged.

predict / ClientReplyRef / ClientStrictRef are reply_ref.predict's walk (and,
for the strict call, fail_ref's failing-item walk in front of it) with the
oracle's client SendFrame builder, orc.OrcTx(is_server=False).frame(p, ft,
last, FWS_TX_FRAG_KEY(key, j)), as the byte builder: they predict every output
of fws_gpu_reply_messages_multi_client / _strict_client for one read.

test_client_cpu.py holds both against the oracle's OnRecvData in the opposite
role."""
import contextlib
import functools
import math
import random
import struct

import numpy as np

import fail_ref
import orc
import reply_ref as rr
import test_gpu_msg_carry as cc
import txmulti_ref as tr
from flashws_amd import _lib
from msgflow_ref import FlowRef
from wsframes import frame

TEXT, BIN, CONT, CLOSE, PING, PONG = 1, 2, 0, 8, 9, 10
MASKED = _lib.FWS_ERR_MASKED
FRAG_KEY = _lib.FWS_TX_FRAG_KEY
ZERO_KEY = bytes(4)


# ------------------------------------------------------------------ the decode
def client_parse(wire):
    """ParseFrameHdr over the stream in the client role (w_socket.h:435-524):
    cc.ref_parse with the role's branch the other way round."""
    frames, pos, n, status = [], 0, len(wire), 0
    while pos < n:
        avail = n - pos
        if avail < 2:
            break
        b0, b1 = wire[pos], wire[pos + 1]
        op = b0 & 15
        if op not in (0, 1, 2, 8, 9, 10):
            status = _lib.FWS_ERR_OPCODE
            break
        if b0 & 0x70:
            status = _lib.FWS_ERR_RSV
            break
        plen, h = b1 & 127, 2
        if plen == 126:
            if avail < 4:
                break
            plen, h = struct.unpack(">H", wire[pos + 2:pos + 4])[0], 4
        elif plen == 127:
            if avail < 10:
                break
            plen, h = struct.unpack(">Q", wire[pos + 2:pos + 10])[0], 10
        if plen > 1 << 32:
            status = _lib.FWS_ERR_TOO_LARGE
            break
        if b1 & 0x80:
            status = MASKED
            break
        frames.append(dict(hdr_off=pos, hdr_len=h, plen=plen, key=ZERO_KEY, op=op, fin=b0 >> 7,
                           trunc=pos + h + plen > n))
        pos += h + plen
    return frames, status


@contextlib.contextmanager
def client_role():
    """FlowRef's walk over the client parse."""
    old, cc.ref_parse = cc.ref_parse, client_parse
    try:
        yield
    finally:
        cc.ref_parse = old


class ClientFlowRef(FlowRef):
    def call(self, wire, *args, **kw):
        with client_role():
            return super().call(wire, *args, **kw)


def whole(stream):
    """The one-call client decode of the whole stream by the walk: (units, status)."""
    out = ClientFlowRef().call(stream)
    return out["units"], out["res"]["status"]


def sframe(opcode, payload, fin=1, len_form=None, rsv=0):
    """A server frame: wsframes.frame without the mask."""
    return frame(opcode, payload, fin=fin, rsv=rsv, masked=False, len_form=len_form)


def to_server_role(wire):
    """A stream of whole server frames as the client frames with the same
    payload bytes: the MASK bit set and a zero key inserted."""
    frames, status = client_parse(wire)
    assert status == 0 and (not frames or not frames[-1]["trunc"])
    out = bytearray()
    for f in frames:
        o, h = f["hdr_off"], f["hdr_len"]
        out += bytes([wire[o], wire[o + 1] | 0x80]) + wire[o + 2:o + h] + ZERO_KEY + wire[o + h:o + h + f["plen"]]
    return bytes(out)


def twelve_frames():
    """cc.twelve_frames as a server writes it: the same twelve frames, length forms and payloads, unmasked."""
    rng = random.Random(2)
    f = [sframe(TEXT, b"he\xe2\x82", fin=0),
         sframe(PING, b"p1"),
         sframe(CONT, b"\xac and more", fin=0, len_form=126),
         sframe(CONT, b"the end \xf0\x9f\x98\x80", fin=1, len_form=127),
         sframe(BIN, b"\x00\xff\x80", fin=0),
         sframe(CONT, b"", fin=0),
         sframe(PONG, b""),
         sframe(CONT, cc.payload(rng, 10), fin=1),
         sframe(TEXT, b"ok"),
         sframe(TEXT, b"bad \xc3("),
         sframe(BIN, cc.payload(rng, 17), len_form=126),
         sframe(CLOSE, struct.pack(">H", 1000) + b"bye")]
    return b"".join(f)


EDGES = (0, 125, 126, 65535, 65536)


def random_server_stream(seed, edges=EDGES):
    """A valid stream of server frames written by the oracle's SendFrame in the
    server role: 20 to 50 frames, fragmented messages, control frames between
    fragments, TEXT bodies well formed or not, payload lengths log-uniform up to
    700 and, every few frames, one of `edges` (seed % len(edges) is always
    there). Returns (wire, the frames' (start, end), the units as (opcode,
    bytes))."""
    rng = random.Random(9000 + seed)
    tx = orc.OrcTx(is_server=True)
    wire, spans, units = bytearray(), [], []
    forced = edges[seed % len(edges)]

    def put(p, ft, last):
        b = tx.frame(p, ft, last, 0)
        spans.append((len(wire), len(wire) + len(b)))
        wire.extend(b)

    target = rng.randint(20, 50)
    while len(spans) < target or forced is not None:
        if rng.random() < 0.1:
            p = cc.payload(rng, rng.choice((0, 125, rng.randint(0, 125))))
            op = rng.choice((PING, PONG))
            put(p, op, 1)
            units.append((op, p))
            continue
        n = int(math.exp(rng.uniform(0.0, math.log(701)))) - 1
        if forced is not None and len(spans) >= 3:
            n, forced = forced, None
        elif rng.random() < 0.12:
            n = rng.choice(edges)
        op = rng.choice((TEXT, BIN)) if n < 4096 else BIN
        body = cc.random_text(rng, n) if op == TEXT else cc.payload(rng, n)
        if op == TEXT and n and rng.random() < 0.15:
            b = bytearray(body)
            b[rng.randrange(n)] = rng.choice((0xFF, 0xC0, 0x80, 0xED, 0xF5))
            body = bytes(b)
        parts = [body]
        if rng.random() < 0.4 or not units:
            cuts = sorted(rng.randint(0, n) for _ in range(rng.randint(1, 5)))
            parts = [body[a:b] for a, b in zip([0] + cuts, cuts + [n])]
        for j, p in enumerate(parts):
            put(p, op, int(j == len(parts) - 1))
            if j + 1 < len(parts) and rng.random() < 0.15:
                c = cc.payload(rng, rng.randint(0, 20))
                put(c, PING, 1)
                units.append((PING, c))
        units.append((op, body))
    return bytes(wire), spans, units


def random_cuts(seed, wire, spans, lo=3, hi=12):
    """lo to hi cut points: one inside a frame's payload where a frame has one, the rest anywhere."""
    rng = random.Random(7000 + seed)
    cuts = {rng.randint(1, len(wire) - 1) for _ in range(rng.randint(lo, hi))}
    inside = [(a, b) for a, b in spans if b - a > 12]
    if inside:
        a, b = rng.choice(inside)
        cuts.add(rng.randint(a + 11, b - 1))
    return sorted(cuts)


# ------------------------------------------------------------------ the replies
def predict(out, flags, tx, state, key=0, msg_cap=rr.BIG, dst_cap=rr.BIG, ctl_cap=rr.BIG, out_cap=None,
            frame_cap=None, out_off=0, conn_ok=True):
    """reply_ref.predict for the client calls: the same walk, every frame built
    by the oracle's client SendFrame with FWS_TX_FRAG_KEY(key, j), the records
    carrying the key."""

    def nothing(status, n_frames=0, out_len=0, lmnf=0):
        return dict(res=tr.refusal(status, n_frames, out_len) | dict(last_msg_not_fin=lmnf), bytes=b"",
                    records=np.zeros(0, dtype=_lib.FRAME_INFO), frames=[], tx=tx, state=state)

    res = out["res"]
    if out_off & 15 or not conn_ok:
        return nothing(rr.INVALID)
    open_now = int(tx["last_msg_not_fin"] != 0)
    undelivered = (res["status"] in (rr.DECLINED, rr.INVALID) or res["n_msgs"] > msg_cap or
                   res["data_bytes"] > dst_cap or res["ctl_bytes"] > ctl_cap)
    if undelivered:
        return nothing(0, lmnf=open_now)
    if res["n_msgs"] > rr.MAX_ENTRIES:
        return nothing(rr.INVALID)
    if state["close_sent"]:
        return nothing(0, lmnf=open_now)
    otx = orc.OrcTx(is_server=False)
    otx.state.value = open_now
    wire, frames, new_state = [], [], state
    want = rr.items(out, flags)
    recs = np.zeros(len(want), dtype=_lib.FRAME_INFO)
    for j, (ft, p, last) in enumerate(want):
        k = FRAG_KEY(key, j)
        b = otx.frame(p, ft, last, k)
        h = tr.hdr_len(len(p), True)
        assert len(b) == h + len(p) and b[1] & 0x80 and b[h - 4:h] == k.to_bytes(4, "little")
        recs[j] = (sum(map(len, wire)), len(p), k, b[0] & 15, b[0] >> 7, h, 0)
        wire.append(b)
        frames.append((b[0] & 15, b[0] >> 7, p))
        if ft == CLOSE:
            code = int.from_bytes(p[:2], "big") if len(p) >= 2 else 1005
            new_state = dict(state, close_sent=1, close_code=code)
    wire = b"".join(wire)
    if out_cap is not None and len(wire) > out_cap:
        return nothing(rr.CAPACITY, len(want), len(wire))
    nxt = dict(tx, last_msg_not_fin=int(otx.state.value), frames=tx["frames"] + len(want),
               wire_bytes=tx["wire_bytes"] + len(wire))
    r = dict(status=0, n_frames=len(want), out_len=len(wire), last_msg_not_fin=nxt["last_msg_not_fin"], pad=0,
             reserved=0)
    shown = len(want) if frame_cap is None else min(len(want), frame_cap)
    return dict(res=r, bytes=wire, records=recs[:shown].copy(), frames=frames, tx=nxt, state=new_state)


@contextlib.contextmanager
def masked_with(key):
    """fail_ref.predict over the client byte builder."""
    old, rr.predict = rr.predict, functools.partial(predict, key=key)
    try:
        yield
    finally:
        rr.predict = old


def predict_strict(out, flags, tx, state, key=0, limit=0, **kw):
    with masked_with(key):
        return fail_ref.predict(out, flags, tx, state, limit=limit, **kw)


class ClientReplyRef(rr.ReplyRef):
    """A client connection's send and reply states by the contract; key is the next call's key for it."""

    def __init__(self, flags):
        super().__init__(flags)
        self.state = fail_ref.new_state()             # (fail_code stays 0)
        self.key = 0

    def predict(self, out, **kw):
        return predict(out, self.flags, self.tx, self.state, key=self.key, **kw)

    def call(self, out, **kw):
        got = self.predict(out, **kw)
        self.tx, self.state = got["tx"], got["state"]
        self.wire += got["bytes"]
        self.frames += got["frames"]
        return got


class ClientStrictRef(ClientReplyRef):
    def __init__(self, flags, limit=0):
        super().__init__(flags)
        self.limit = limit

    def predict(self, out, **kw):
        return predict_strict(out, self.flags, self.tx, self.state, key=self.key, limit=self.limit, **kw)


def walk_client_frames(wire):
    """Masked frames back to back: [(opcode, fin, payload unmasked, key)].
    Asserts client frames (MASK bit, no RSV, minimal length forms) that end
    exactly at the end."""
    out, pos = [], 0
    while pos < len(wire):
        b0, b1 = wire[pos], wire[pos + 1]
        assert not b0 & 0x70 and b1 & 0x80, pos
        n, pos = b1 & 127, pos + 2
        if n == 126:
            n, pos = int.from_bytes(wire[pos:pos + 2], "big"), pos + 2
            assert n >= 126
        elif n == 127:
            n, pos = int.from_bytes(wire[pos:pos + 8], "big"), pos + 8
            assert n > 65535
        key, pos = int.from_bytes(wire[pos:pos + 4], "little"), pos + 4
        assert pos + n <= len(wire)
        raw = np.frombuffer(wire[pos:pos + n], dtype=np.uint8)
        k = np.frombuffer(key.to_bytes(4, "little") * (n // 4 + 1), dtype=np.uint8)[:n]
        out.append((b0 & 15, b0 >> 7, (raw ^ k).tobytes(), key))
        pos += n
    return out
