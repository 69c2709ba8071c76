"""Host model of fws_gpu_publish_messages (include/fws_gpu.h): from a
connection's tx state and reply state, the records, the three buffers they name,
the subscriber's list and its capacities it predicts the region's bytes, the
fws_tx_result, the frame records and both next states. Every frame's bytes come
from the oracle's SendFrame builder, orc.OrcTx(is_server=True).frame(), one per
frame, which tests/golden/tx_cases.json.gz pins to the reference (through
txmulti_ref, test_publish_cpu.py); the items, the refusals and their order are
the header's contract restated. The GPU tests have no other oracle."""
import ctypes as C

import numpy as np

import orc
import txmulti_ref as tr
from flashws_amd import _lib

TEXT, BIN, CLOSE, PING, PONG = 1, 2, 8, 9, 10
INVALID, CONTROL, DECLINED, SEQUENCE, CAPACITY = (_lib.FWS_ERR_INVALID, _lib.FWS_ERR_CONTROL_FRAME,
                                                  _lib.FWS_ERR_DECLINED, _lib.FWS_ERR_SEQUENCE, _lib.FWS_ERR_CAPACITY)
IN_DST, IN_STORE, IN_CTL, NOWHERE = (_lib.FWS_JOIN_IN_DST, _lib.FWS_JOIN_IN_STORE, _lib.FWS_JOIN_IN_CTL,
                                     _lib.FWS_JOIN_NOWHERE)
MAX_ITEMS, MAX_SEND = _lib.FWS_PUB_MAX_ITEMS, _lib.FWS_TX_MULTI_MAX_SEND

new_tx = tr.new_state
tx_bytes = tr.state_bytes


def new_state():
    return dict(close_sent=0, close_code=0, fail_code=0, reserved=0)


def state_bytes(state):
    rec = np.zeros(1, dtype=_lib.REPLY_STATE)
    for k, v in state.items():
        rec[0][k] = v
    return rec.tobytes()


def records(items):
    """JOIN_INFO records from (opcode, where, off, len) tuples."""
    recs = np.zeros(len(items), dtype=_lib.JOIN_INFO)
    for i, (op, where, off, ln) in enumerate(items):
        recs[i]["opcode"], recs[i]["where"], recs[i]["off"], recs[i]["len"] = op, where, off, ln
    return recs


def is_nothing(rec):
    return int(rec["opcode"]) == 0 or int(rec["where"]) == NOWHERE


def frame(otx, payload, op):
    """One whole frame from the oracle's builder: otx.frame(), or for a large
    payload the same orc_tx_frame call on numpy buffers (frame() goes through
    Python lists, a second per megabyte)."""
    if len(payload) <= 4096:
        return otx.frame(payload, op, 1, 0)
    src = np.frombuffer(payload, dtype=np.uint8)
    out = np.empty(len(payload) + 14, dtype=np.uint8)
    k = orc.orc().orc_tx_frame(C.byref(otx.state), otx.is_server, src.ctypes.data, len(payload), op, 1, 0,
                               out.ctypes.data)
    return out[:k].tobytes()


def predict(tx, state, recs, bases, lst, max_len=MAX_SEND, out_cap=None, frame_cap=None, out_off=0, conn_ok=True,
            list_ok=True, cache=None):
    """One subscriber. recs: the call's JOIN_INFO records; bases: (dst, store,
    ctl) as bytes-like, None for a base passed as NULL; lst: the subscriber's
    indices. list_ok False: list_off + list_len > n_list. cache (a dict) keeps
    frames by (opcode, where, off, len) between calls over the same buffers.
    Returns dict(res, bytes, records, frames, tx, state): the fws_tx_result's
    fields, the region's bytes, the FRAME_INFO records written, the frames as
    (opcode, fin, payload) and the two states after the call (the arguments
    themselves when nothing changed)."""

    def nothing(status, n_frames=0, out_len=0, lmnf=0):
        return dict(res=tr.refusal(status, n_frames, out_len) | dict(last_msg_not_fin=lmnf), bytes=b"",
                    records=np.zeros(0, dtype=_lib.FRAME_INFO), frames=[], tx=tx, state=state)

    # 1. invalid
    if out_off & 15 or not conn_ok or len(lst) > MAX_ITEMS or not list_ok:
        return nothing(INVALID)
    judged = []
    for i in lst:
        if i >= len(recs):
            return nothing(INVALID)
        r = recs[i]
        if is_nothing(r):
            continue
        op, where = int(r["opcode"]), int(r["where"])
        if op not in (TEXT, BIN, CLOSE, PING, PONG) or where > 3 or bases[where] is None:
            return nothing(INVALID)
        judged.append((op, where, int(r["off"]), int(r["len"])))
    # 2. no frames
    open_now = int(tx["last_msg_not_fin"] != 0)
    if state["close_sent"] or not judged:
        return nothing(0, lmnf=open_now)
    # 3, 4. every record is judged, behind a CLOSE or not
    if any(op >= 8 and ln > 125 for op, _, _, ln in judged):
        return nothing(CONTROL)
    if any(op < 8 and (ln > max_len or ln > MAX_SEND) for op, _, _, ln in judged):
        return nothing(DECLINED)
    # the frames that would be written: up to and including the first CLOSE
    want = []
    for it in judged:
        want.append(it)
        if it[0] == CLOSE:
            break
    # 5. a whole message is not cut into an open one
    if open_now and any(op < 8 for op, _, _, _ in want):
        return nothing(SEQUENCE)
    otx = orc.OrcTx(is_server=True)
    otx.state.value = open_now
    wire, frames, at = [], [], 0
    out_recs = np.zeros(len(want), dtype=_lib.FRAME_INFO)
    for j, it in enumerate(want):
        op, where, off, ln = it
        got = cache.get(it) if cache is not None else None
        if got is None:
            p = bytes(bases[where][off:off + ln])
            assert len(p) == ln, "a record past the end of its buffer"
            b = frame(otx, p, op)
            assert len(b) == tr.hdr_len(ln, False) + ln and b[len(b) - ln:] == p and b[0] == 0x80 | op
            got = (b, p)
            if cache is not None:
                cache[it] = got
        b, p = got
        out_recs[j] = (at, ln, 0, op, 1, len(b) - ln, 0)
        wire.append(b)
        frames.append((op, 1, p))
        at += len(b)
    assert otx.state.value == open_now            # whole messages and control frames leave it as it was
    # 6. capacity
    if out_cap is not None and at > out_cap:
        return nothing(CAPACITY, len(want), at)
    wire = b"".join(wire)
    nxt = dict(tx, frames=tx["frames"] + len(want), wire_bytes=tx["wire_bytes"] + at)
    nstate = dict(state, close_sent=1) if want[-1][0] == CLOSE else state
    res = dict(status=0, n_frames=len(want), out_len=at, last_msg_not_fin=open_now, pad=0, reserved=0)
    shown = len(want) if frame_cap is None else min(len(want), frame_cap)
    return dict(res=res, bytes=wire, records=out_recs[:shown].copy(), frames=frames, tx=nxt, state=nstate)
