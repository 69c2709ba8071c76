"""StrictRef: the host walk that predicts every output of
fws_gpu_reply_messages_strict for one read (include/fws_gpu.h). It is
reply_ref.predict with the failing-item walk of the header's table in front:
the read's items -- its entries, the open part, the decode's error -- each get a
failure code or none, from the entry, the decode's result, the connection's
decode state (FlowRef's state dict or RefConn's carry dict, as the decode
reference returned it for this read) and, for a CLOSE reason, Python's strict
decoder. With a failing item f at or before the first CLOSE answered, the
frames asked for are those of the items before f and one CLOSE whose payload is
the code; predict then sequences and builds them exactly as for the plain call.
The oracle has no failing semantics, so the table is the yardstick and this
file restates it."""
import contextlib

import reply_ref as rr
import txmulti_ref as tr
from flashws_amd import _lib
from reply_ref import BIN, CLOSE, CONTROL, ECHO, PING, PONG, TEXT

PROTOCOL, BAD_DATA, TOO_BIG = 1002, 1007, 1009
MAX_FRAMES_OUT = _lib.FWS_MSG_MULTI_MAX_FRAMES + 2       # the frame table's size
CONTINUED = _lib.FWS_MSG_CONTINUED


def code_valid(c):
    """May c appear in a CLOSE frame: 1000-1003, 1007-1014, 3000-4999."""
    return 1000 <= c <= 1003 or 1007 <= c <= 1014 or 3000 <= c <= 4999


def utf8(b):
    try:
        bytes(b).decode("utf-8", "strict")
        return True
    except UnicodeDecodeError:
        return False


def carry_of(out):
    """(the fws_msg_carry fields, frame_unread) of a decode reference's output."""
    if "state" in out:                                # FlowRef
        return out["state"]["msg"], out["state"]["frame_unread"]
    if "carry" in out:                                # RefConn
        return out["carry"], 0
    return dict.fromkeys(_lib.MSG_CARRY.names, 0), 0  # an undecoded read: never looked at


def close_failure(payload):
    n = len(payload)
    if n == 0:
        return 0
    if n == 1 or not code_valid(int.from_bytes(payload[:2], "big")):
        return PROTOCOL
    return 0 if utf8(payload[2:]) else BAD_DATA


def failures(out, limit):
    """[(item index, code)] of the read's failing items, in order. Only the
    read's first CLOSE entry is judged."""
    res, (carry, unread) = out["res"], carry_of(out)
    got, seen_close = [], False
    for i, e in enumerate(out["entries"]):
        op, code = e["opcode"], 0
        if op in (TEXT, BIN):
            before = carry["prev_open_bytes"] if e["flags"] & CONTINUED else 0
            if limit and before + e["len"] > limit:
                code = TOO_BIG
            elif op == TEXT and not e["utf8_ok"]:
                code = BAD_DATA
        elif op == CLOSE and not seen_close and e["len"] <= 125:
            seen_close = True
            code = close_failure(out["ctl"][e["off"]:e["off"] + e["len"]])
        if code:
            got.append((i, code))
    n = len(out["entries"])
    if limit and carry["open_bytes"] + unread > limit:
        got.append((n, TOO_BIG))
    elif res["open_opcode"] == TEXT and carry["utf8_bad"]:
        got.append((n, BAD_DATA))
    if res["status"] == _lib.FWS_ERR_TOO_LARGE:
        got.append((n + 1, TOO_BIG))
    elif res["status"] in _lib.FWS_PROTOCOL_ERRORS:
        got.append((n + 1, PROTOCOL))
    return got


def first_close_answered(out, flags):
    if flags & CONTROL:
        for i, e in enumerate(out["entries"]):
            if e["opcode"] == CLOSE:
                return i
    return None


def failing_items(out, flags, f, code):
    """reply_ref.items with item f replaced by the failing CLOSE and nothing behind it."""
    res, got = out["res"], []
    for i, e in enumerate(out["entries"]):
        if i == f:
            break
        op, o, n = e["opcode"], e["off"], e["len"]
        if op == PING and flags & CONTROL:
            got.append((PONG, out["ctl"][o:o + n], 1))
        elif op in (TEXT, BIN) and flags & ECHO:
            got.append((op, out["dst"][o:o + n], 1))
    if f > len(out["entries"]) and flags & ECHO and res["open_opcode"] and res["open_len"]:
        o = res["open_off"]
        got.append((res["open_opcode"], out["dst"][o:o + res["open_len"]], 0))
    got.append((CLOSE, code.to_bytes(2, "big"), 1))
    return got


@contextlib.contextmanager
def items_are(want):
    """reply_ref.predict over a given list of frames."""
    old, rr.items = rr.items, lambda out, flags: want
    try:
        yield
    finally:
        rr.items = old


def new_state():
    return dict(rr.new_state(), fail_code=0)


def predict(out, flags, tx, state, limit=0, **kw):
    """One read: reply_ref.predict's dict; state has fail_code."""
    fails = failures(out, limit)
    c = first_close_answered(out, flags)
    if not fails or (c is not None and c < fails[0][0]):
        return rr.predict(out, flags, tx, state, **kw)
    f, code = fails[0]
    want = failing_items(out, flags, f, code)
    with items_are(want):
        got = rr.predict(out, flags, tx, state, **kw)
    if not got["res"]["n_frames"]:                    # an earlier refusal or nothing to say: the walk was not reached
        return got
    if len(want) > MAX_FRAMES_OUT:                    # 257 entries, an open part and an error: not a decode output
        return dict(got, res=tr.refusal(_lib.FWS_ERR_INVALID) | dict(last_msg_not_fin=0), bytes=b"", frames=[],
                    records=got["records"][:0], tx=tx, state=state)
    if got["res"]["status"]:
        return got
    new = dict(state, close_sent=1, fail_code=code)
    if f < len(out["entries"]) and out["entries"][f]["opcode"] == CLOSE:
        e = out["entries"][f]
        p = out["ctl"][e["off"]:e["off"] + e["len"]]
        new["close_code"] = int.from_bytes(p[:2], "big") if len(p) >= 2 else 1005
    return dict(got, state=new)


class StrictRef(rr.ReplyRef):
    """A connection's send and reply states by the strict call's contract."""

    def __init__(self, flags, limit=0):
        super().__init__(flags)
        self.state, self.limit = new_state(), limit

    def call(self, out, **kw):
        got = predict(out, self.flags, self.tx, self.state, limit=self.limit, **kw)
        self.tx, self.state = got["tx"], got["state"]
        self.wire += got["bytes"]
        self.frames += got["frames"]
        return got
