"""ReplyRef: the host walk that predicts every output of
fws_gpu_reply_messages_multi for one read (include/fws_gpu.h) -- the region's
bytes, the frame records, the fws_tx_result and both states -- from what the
decode delivered for the read (a FlowRef.call / RefConn.call output), the flags
and the connection's two states. The items are walked in order, one
fws_tx_next step per data frame, and every frame's bytes come from the
oracle's SendFrame builder, orc.OrcTx(is_server=True).frame(), which
tests/golden/tx_cases.json.gz pins to the reference; the selection of items and
the refusals are the header's contract restated. test_reply_cpu.py holds the
walk against the oracle's OnRecvData."""
import numpy as np

import orc
import txmulti_ref as tr
from flashws_amd import _lib

CONTROL, ECHO = _lib.FWS_REPLY_CONTROL, _lib.FWS_REPLY_ECHO
TEXT, BIN, CLOSE, PING, PONG = 1, 2, 8, 9, 10
INVALID, CAPACITY, DECLINED = _lib.FWS_ERR_INVALID, _lib.FWS_ERR_CAPACITY, _lib.FWS_ERR_DECLINED
MAX_ENTRIES = _lib.FWS_MSG_MULTI_MAX_FRAMES + 1
BIG = 1 << 30

new_tx = tr.new_state
tx_bytes = tr.state_bytes


def new_state():
    return dict(close_sent=0, close_code=0, reserved=0)


def state_bytes(state):
    rec = np.zeros(1, dtype=_lib.REPLY_STATE)
    for k, v in state.items():
        rec[0][k] = v
    return rec.tobytes()


def undecoded(status):
    """What a declined or invalid read looks like to the reply: its fws_msg_result."""
    res = dict.fromkeys(_lib.MSG_RESULT.names, 0)
    res.update(status=status, err_frame=0xFFFFFFFF, open_first_frame=0xFFFFFFFF)
    return dict(res=res, entries=[], dst=b"", ctl=b"")


def items(out, flags):
    """The frames the read asks for, before sequencing: (frame_type, payload, last) in order, up to and
    including the first CLOSE answered."""
    res, got = out["res"], []
    for e in out["entries"]:
        op, o, n = e["opcode"], e["off"], e["len"]
        if op == PING and flags & CONTROL:
            got.append((PONG, out["ctl"][o:o + n], 1))
        elif op == CLOSE and flags & CONTROL:
            got.append((CLOSE, out["ctl"][o:o + n], 1))
            return got
        elif op in (TEXT, BIN) and flags & ECHO:
            got.append((op, out["dst"][o:o + n], 1))
    if flags & ECHO and res["open_opcode"] and res["open_len"]:
        o = res["open_off"]
        got.append((res["open_opcode"], out["dst"][o:o + res["open_len"]], 0))
    return got


def predict(out, flags, tx, state, msg_cap=BIG, dst_cap=BIG, ctl_cap=BIG, out_cap=None, frame_cap=None, out_off=0,
            conn_ok=True):
    """One read. Returns dict(res, bytes, records, frames, tx, state): the
    fws_tx_result's fields, the region's bytes, the FRAME_INFO records written,
    the frames as (opcode, fin, payload), and the two states after the call (the
    arguments themselves when nothing changed)."""

    def nothing(status, n_frames=0, out_len=0, lmnf=0):
        return dict(res=tr.refusal(status, n_frames, out_len) | dict(last_msg_not_fin=lmnf), bytes=b"",
                    records=np.zeros(0, dtype=_lib.FRAME_INFO), frames=[], tx=tx, state=state)

    res = out["res"]
    if out_off & 15 or not conn_ok:
        return nothing(INVALID)
    open_now = int(tx["last_msg_not_fin"] != 0)
    undelivered = (res["status"] in (DECLINED, INVALID) or res["n_msgs"] > msg_cap or res["data_bytes"] > dst_cap or
                   res["ctl_bytes"] > ctl_cap)
    if undelivered:
        return nothing(0, lmnf=open_now)
    if res["n_msgs"] > MAX_ENTRIES:
        return nothing(INVALID)
    if state["close_sent"]:
        return nothing(0, lmnf=open_now)
    otx = orc.OrcTx(is_server=True)
    otx.state.value = open_now
    wire, frames, new_state_ = [], [], state
    want = items(out, flags)
    recs = np.zeros(len(want), dtype=_lib.FRAME_INFO)
    for j, (ft, p, last) in enumerate(want):
        b = otx.frame(p, ft, last, 0)
        assert len(b) == tr.hdr_len(len(p), False) + len(p) and b[len(b) - len(p):] == p
        recs[j] = (sum(map(len, wire)), len(p), 0, b[0] & 15, b[0] >> 7, len(b) - len(p), 0)
        wire.append(b)
        frames.append((b[0] & 15, b[0] >> 7, p))
        if ft == CLOSE:
            code = int.from_bytes(p[:2], "big") if len(p) >= 2 else 1005
            new_state_ = dict(state, close_sent=1, close_code=code)
    wire = b"".join(wire)
    if out_cap is not None and len(wire) > out_cap:
        return nothing(CAPACITY, len(want), len(wire))
    nxt = dict(tx, last_msg_not_fin=int(otx.state.value), frames=tx["frames"] + len(want),
               wire_bytes=tx["wire_bytes"] + len(wire))
    r = dict(status=0, n_frames=len(want), out_len=len(wire), last_msg_not_fin=nxt["last_msg_not_fin"], pad=0,
             reserved=0)
    shown = len(want) if frame_cap is None else min(len(want), frame_cap)
    return dict(res=r, bytes=wire, records=recs[:shown].copy(), frames=frames, tx=nxt, state=new_state_)


class ReplyRef:
    """A connection's send and reply states by the contract, advanced call by call."""

    def __init__(self, flags):
        self.flags, self.tx, self.state = flags, new_tx(), new_state()
        self.wire, self.frames = b"", []

    def call(self, out, **kw):
        got = predict(out, self.flags, self.tx, self.state, **kw)
        self.tx, self.state = got["tx"], got["state"]
        self.wire += got["bytes"]
        self.frames += got["frames"]
        return got


def walk_frames(wire):
    """Unmasked frames back to back: [(opcode, fin, payload)]. Asserts server
    frames (no MASK bit, no RSV) that end exactly at the end."""
    out, pos = [], 0
    while pos < len(wire):
        b0, b1 = wire[pos], wire[pos + 1]
        assert not b0 & 0x70 and not b1 & 0x80, pos
        n, pos = b1 & 127, pos + 2
        if n == 126:
            n, pos = int.from_bytes(wire[pos:pos + 2], "big"), pos + 2
            assert n >= 126
        elif n == 127:
            n, pos = int.from_bytes(wire[pos:pos + 8], "big"), pos + 8
            assert n > 65535
        assert pos + n <= len(wire)
        out.append((b0 & 15, b0 >> 7, wire[pos:pos + n]))
        pos += n
    return out


def messages(frames):
    """The frames as a receiver sees them: [(opcode, payload)] of control frames
    and of data messages joined over their fragments, in completion order.
    Asserts RFC 6455 sequencing: no continuation without an open message, no
    TEXT / BIN inside one, control frames whole, nothing after a CLOSE. Returns
    (units, the open message's (opcode, bytes so far) or None)."""
    units, cur, closed = [], None, False
    for op, fin, p in frames:
        assert not closed, "a frame after the CLOSE"
        if op >= 8:
            assert fin and len(p) <= 125 and op in (CLOSE, PING, PONG)
            units.append((op, p))
            closed = op == CLOSE
            continue
        if op == 0:
            assert cur is not None, "a continuation with no message open"
            cur = (cur[0], cur[1] + p)
        else:
            assert cur is None and op in (TEXT, BIN), "a new message inside an open one"
            cur = (op, p)
        if fin:
            units.append(cur)
            cur = None
    return units, cur
