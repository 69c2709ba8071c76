"""Host model of fws_gpu_encode_messages_multi (include/fws_gpu.h): from a
connection's state, a send and its capacities it predicts the region's bytes,
the fws_tx_result, the frame records and the next state. The bytes come from
the oracle's SendFrame builder, one orc.OrcTx.frame() per fragment, started
from the state's last_msg_not_fin; the cutting, the keys and the refusals are
the header's contract restated. The GPU tests have no other oracle;
test_tx_multi_cpu.py holds this model against the reference's recorded frames."""
import numpy as np

import orc
from flashws_amd import _lib

TEXT, BIN, CLOSE, PING, PONG = 1, 2, 8, 9, 10
INVALID, CONTROL, DECLINED, CAPACITY = (_lib.FWS_ERR_INVALID, _lib.FWS_ERR_CONTROL_FRAME, _lib.FWS_ERR_DECLINED,
                                        _lib.FWS_ERR_CAPACITY)
MAX_SEND, MAX_FRAMES = _lib.FWS_TX_MULTI_MAX_SEND, _lib.FWS_TX_MULTI_MAX_FRAMES
frag_key = _lib.FWS_TX_FRAG_KEY


def new_state():
    return dict(last_msg_not_fin=0, reserved0=0, frames=0, wire_bytes=0, reserved=0)


def state_bytes(state):
    rec = np.zeros(1, dtype=_lib.TX_CONN)
    for k, v in state.items():
        rec[0][k] = v
    return rec.tobytes()


def slices(n, max_frame, control=False):
    """(offset, length) of the payload slices a send of n bytes is cut into."""
    if control or max_frame == 0 or n <= max_frame:
        return [(0, n)]
    return [(o, min(max_frame, n - o)) for o in range(0, n, max_frame)]


def hdr_len(n, masked):
    return 2 + (4 if masked else 0) + (0 if n < 126 else 2 if n <= 65535 else 8)


def refusal(status, n_frames=0, out_len=0):
    return dict(status=status, n_frames=n_frames, out_len=out_len, last_msg_not_fin=0, pad=0, reserved=0)


def predict(state, payload, frame_type, last, masked=True, key=0, max_frame=0, out_cap=None, frame_cap=None,
            max_len=MAX_SEND, out_off=0, conn_ok=True, max_send=MAX_SEND):
    """One send. Returns dict(res, bytes, records, state): the fws_tx_result's
    fields, the region's bytes (b"" when refused), the FRAME_INFO records
    written (min(n_frames, frame_cap) of them) and the state after the send
    (the argument itself, unchanged, when refused). max_send: the call's limit
    on a send, lifted only to hold the model's bytes against recorded frames
    that are larger than one call takes."""
    n = len(payload)
    control = bool(frame_type & 8)

    def refused(status, n_frames=0, out_len=0):
        return dict(res=refusal(status, n_frames, out_len), bytes=b"", records=np.zeros(0, dtype=_lib.FRAME_INFO),
                    state=state)

    if out_off & 15 or not conn_ok or frame_type not in (TEXT, BIN, CLOSE, PING, PONG):
        return refused(INVALID)
    if control and n > 125:
        return refused(CONTROL)
    if n > max_len or n > max_send:
        return refused(DECLINED)
    cut = slices(n, max_frame, control)
    k = len(cut)
    if k > MAX_FRAMES:
        return refused(DECLINED)
    need = sum(hdr_len(ln, masked) + ln for _, ln in cut)
    if out_cap is not None and need > out_cap:
        return refused(CAPACITY, k, need)
    tx = orc.OrcTx(is_server=not masked)
    tx.state.value = int(state["last_msg_not_fin"])
    wire, recs = [], np.zeros(k, dtype=_lib.FRAME_INFO)
    for j, (o, ln) in enumerate(cut):
        fkey = frag_key(key, j) if masked else 0
        b = tx.frame(payload[o:o + ln], frame_type, bool(last) and j == k - 1, fkey)
        assert len(b) == hdr_len(ln, masked) + ln
        recs[j] = (sum(map(len, wire)), ln, fkey, b[0] & 15, b[0] >> 7, len(b) - ln, 0)
        wire.append(b)
    wire = b"".join(wire)
    assert len(wire) == need
    nxt = dict(state, last_msg_not_fin=int(tx.state.value), frames=state["frames"] + k,
               wire_bytes=state["wire_bytes"] + need)
    res = dict(status=0, n_frames=k, out_len=need, last_msg_not_fin=nxt["last_msg_not_fin"], pad=0, reserved=0)
    shown = k if frame_cap is None else min(k, frame_cap)
    return dict(res=res, bytes=wire, records=recs[:shown].copy(), state=nxt)
