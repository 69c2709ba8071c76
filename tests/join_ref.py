"""JoinRef: the host model of fws_gpu_join_messages for one connection
(include/fws_gpu.h) over what FlowRef.call (msgflow_ref.py) or RefConn.call
returns for a read: the 32-byte state, the bytes of the connection's slot, and
per call the records and the result. The rules are the header's, in its order;
nothing here looks at how the kernel does it."""
import numpy as np

from flashws_amd import _lib

IN_DST, IN_STORE, IN_CTL, NOWHERE = (_lib.FWS_JOIN_IN_DST, _lib.FWS_JOIN_IN_STORE, _lib.FWS_JOIN_IN_CTL,
                                     _lib.FWS_JOIN_NOWHERE)
DROPPED = _lib.FWS_JOIN_DROPPED
CONTINUED = _lib.FWS_MSG_CONTINUED
MAX_READ, MAX_FRAMES = _lib.FWS_MSG_MULTI_MAX_READ, _lib.FWS_MSG_MULTI_MAX_FRAMES
INVALID = _lib.FWS_ERR_INVALID
BIG = 1 << 40
ZERO_STATE = dict.fromkeys(_lib.JOIN_STATE.names, 0)
ZERO_RESULT = dict.fromkeys(_lib.JOIN_RESULT.names, 0)


def state_bytes(state):
    rec = np.zeros(1, dtype=_lib.JOIN_STATE)
    for k, v in state.items():
        rec[0][k] = v
    return rec.tobytes()


def result_bytes(res):
    rec = np.zeros(1, dtype=_lib.JOIN_RESULT)
    for k, v in res.items():
        rec[0][k] = v
    return rec.tobytes()


def records_bytes(records):
    rec = np.zeros(len(records), dtype=_lib.JOIN_INFO)
    for i, r in enumerate(records):
        for k, v in r.items():
            rec[i][k] = v
    return rec.tobytes()


def undecoded(status):
    """What a declined or refused read leaves: the status, every count zero."""
    return dict(res=dict(status=status, n_msgs=0, open_opcode=0, data_bytes=0, ctl_bytes=0, open_off=0, open_len=0),
                entries=[], dst=b"", ctl=b"")


class JoinRef:
    """One connection: H bytes to a half, the slot pre-filled with `fill`.
    window: the bytes of each half that are modelled (a slot of gigabytes is not
    held whole); slot is the two windows back to back."""

    def __init__(self, H, fill=0, window=None):
        self.H = H
        self.W = H if window is None else min(H, window)
        self.state = dict(ZERO_STATE)
        self.slot = bytearray([fill]) * (2 * self.W)

    def _append(self, st, part):
        p = len(part)
        st["open_bytes"] += p
        if st["dropped"]:
            return 0
        if st["fill"] + p > self.H:
            st["dropped"], st["fill"] = 1, 0
            return 0
        assert st["fill"] + p <= self.W, "an append past the modelled window"
        at = st["half"] * self.W + st["fill"]
        self.slot[at:at + p] = part
        st["fill"] += p
        return p

    def call(self, out, dst_off=0, ctl_off=0, slot_off=0, msg_cap=BIG, dst_cap=BIG, ctl_cap=BIG, conn_ok=True):
        """The read's result and records; the state and the slot advance unless the read is refused.
        out: res / entries / dst of the decode; dst_off, ctl_off: the read's regions; slot_off: conn * store_stride."""
        r, entries, dst = out["res"], out["entries"], out["dst"]
        refused = dict(res=dict(ZERO_RESULT, status=INVALID), records=[])
        if not conn_ok:
            return refused
        S = self.state
        if r["status"] in (_lib.FWS_ERR_DECLINED, INVALID) or r["n_msgs"] > msg_cap or r["data_bytes"] > dst_cap or \
                r["ctl_bytes"] > ctl_cap:
            return dict(res=dict(ZERO_RESULT, open_opcode=S["open_opcode"], dropped=S["dropped"]), records=[])
        if r["n_msgs"] > MAX_FRAMES + 1:
            return refused
        entries = entries[:r["n_msgs"]]
        data = [i for i, e in enumerate(entries) if e["opcode"] < 8]
        cont = [i for i in data if entries[i]["flags"] & CONTINUED]
        if any(entries[i]["len"] > MAX_READ for i in data) or (r["open_opcode"] and r["open_len"] > MAX_READ) or \
                S["open_opcode"] > 2:
            return refused
        if cont and (S["open_opcode"] == 0 or len(cont) > 1 or cont[0] != data[0]):
            return refused
        if S["open_opcode"] and not cont and (data or r["open_opcode"] != S["open_opcode"]):
            return refused
        st, records, copied = dict(S), [], 0
        for e in entries:
            rec = dict(off=0, len=e["len"], opcode=e["opcode"], utf8_ok=0, where=IN_CTL, flags=0, reserved0=0,
                       reserved=0)
            if e["opcode"] >= 8:
                rec.update(off=ctl_off + e["off"])
            elif not e["flags"] & CONTINUED:
                rec.update(where=IN_DST, off=dst_off + e["off"], utf8_ok=e["utf8_ok"])
            else:
                copied += self._append(st, dst[:e["len"]])
                if st["dropped"]:
                    rec.update(where=NOWHERE, off=0, len=st["open_bytes"], flags=DROPPED, utf8_ok=e["utf8_ok"])
                else:
                    rec.update(where=IN_STORE, off=slot_off + st["half"] * self.H, len=st["fill"],
                               utf8_ok=e["utf8_ok"])
                    st["half"] ^= 1
                st.update(open_opcode=0, dropped=0, open_bytes=0, fill=0)
            records.append(rec)
        if r["open_opcode"]:
            if st["open_opcode"] == 0:
                st.update(open_opcode=r["open_opcode"], dropped=0, open_bytes=0, fill=0)
            copied += self._append(st, dst[r["open_off"]:r["open_off"] + r["open_len"]])
        self.state = st
        res = dict(ZERO_RESULT, n_joined=len(records), copied=copied, open_opcode=st["open_opcode"],
                   dropped=st["dropped"])
        return dict(res=res, records=records)

    def stored(self, rec, slot_off=0):
        """The bytes an IN_STORE record names, as the slot holds them now."""
        at = (rec["off"] - slot_off) // self.H * self.W
        return bytes(self.slot[at:at + rec["len"]])
