"""FlowRef: the host walk that predicts every output of one
fws_gpu_decode_messages_flow call -- the frame slice, the entries, the dst / ctl
bytes, both results and the 96-byte state -- from the state, the read's bytes
and the four capacities. It is RefConn of test_gpu_msg_carry.py (whose parse,
unmask and UTF-8 rules it uses) with a data frame in progress: the lead, the
cut last data frame, the stop at header FWS_MSG_MULTI_MAX_FRAMES + 1."""
import numpy as np

import test_gpu_msg_carry as cc
from flashws_amd import _lib

NONE, BIG, TEXT = cc.NONE, cc.BIG, cc.TEXT
CONTINUED = _lib.FWS_MSG_CONTINUED
MAX_FRAMES = _lib.FWS_MSG_MULTI_MAX_FRAMES
FRAME_FIELDS = ("frame_unread", "frame_len", "frame_key", "frame_fin")
ZERO_FRAME = dict.fromkeys(FRAME_FIELDS, 0)


def rotr(v, bits):
    bits &= 31
    return ((v >> bits) | (v << (32 - bits))) & 0xFFFFFFFF


def unmask_with(raw, key):
    """raw XORed with the little-endian bytes of key from phase 0."""
    a = np.frombuffer(bytes(raw), dtype=np.uint8)
    k = np.frombuffer(key.to_bytes(4, "little") * (len(a) // 4 + 1), dtype=np.uint8)[:len(a)]
    return (a ^ k).tobytes()


def state_bytes(state):
    """The 96 bytes of fws_msg_flow for a FlowRef state."""
    rec = np.zeros(1, dtype=_lib.MSG_FLOW)
    for k in _lib.MSG_CARRY.names:
        rec[0]["msg"][k] = state["msg"][k]
    for k in FRAME_FIELDS:
        rec[0][k] = state[k]
    return rec.tobytes()


class FlowRef:
    """A connection's state by the contract: msg (the fws_msg_carry fields), the
    four frame fields, and -- the oracle's own -- the open message's bytes."""

    def __init__(self):
        self.state = dict(ZERO_FRAME, msg=dict(cc.ZERO_CARRY))
        self.body = b""

    def call(self, wire, cap=BIG, msg_cap=BIG, dst_cap=BIG, ctl_cap=BIG):
        wire = bytes(wire)
        n = len(wire)
        st, c = self.state, self.state["msg"]
        is_open, opcode, total_frames = c["open_opcode"] != 0, c["open_opcode"], c["open_frames"]
        body = bytearray(self.body)
        continued, first, start, nfrag = is_open, NONE, 0, 0
        dst, ctl, entries, units = bytearray(), bytearray(), [], []
        n_data, err_frame, err_status, resume = 0, NONE, 0, 0
        new_frame = dict(ZERO_FRAME)
        dres = dict.fromkeys(_lib.DECODE_RESULT.names, 0)
        bad = c["utf8_bad"]                           # cc.prefix_bad(body), kept up as the bytes arrive

        def add(p):
            """p to dst and to the open message; an error at one of p's positions sets bad (a position's
            flag depends on the three bytes before it only)."""
            nonlocal bad
            lo = max(0, len(body) - 3)
            dst.extend(p)
            body.extend(p)
            if opcode == TEXT and not bad:
                t = bytes(body[lo:])
                bad = int(any(cc.utf8_flagged(t, j) for j in range(len(t) - len(p), len(t))))

        def complete(last):
            nonlocal is_open, continued, first, body, total_frames, bad
            bad = 0
            ok = cc.strict_ok(body) if opcode == TEXT else 0
            entries.append(dict(off=start, len=len(dst) - start, first_frame=first, last_frame=last,
                                n_data_frames=nfrag, opcode=opcode, utf8_ok=ok,
                                flags=CONTINUED if continued else 0, pad=0))
            units.append((opcode, bytes(body), ok, total_frames))
            is_open, continued, first, body, total_frames = False, False, NONE, bytearray(), 0

        # the lead: payload of the frame in progress
        fu = st["frame_unread"]
        lead = min(fu, n)
        frames, parse_status, capped = [], 0, False
        if fu:
            add(unmask_with(wire[:lead], st["frame_key"]))
            resume = lead
        if fu > n:                                    # the read is all payload
            new_frame = dict(frame_unread=fu - n, frame_len=st["frame_len"],
                             frame_key=rotr(st["frame_key"], 8 * (n & 3)), frame_fin=st["frame_fin"])
            dres.update(consumed=n, carry_unread=fu - n)
        else:
            if fu and st["frame_fin"]:
                complete(NONE)
            frames, parse_status = cc.ref_parse(wire[lead:])
            for f in frames:
                f["hdr_off"] += lead
                f["trunc"] = f["hdr_off"] + f["hdr_len"] + f["plen"] > n
            if len(frames) > MAX_FRAMES:              # the walk stops at header MAX_FRAMES + 1
                frames, parse_status, capped = frames[:MAX_FRAMES + 1], 0, True
            pos = frames[-1]["hdr_off"] + frames[-1]["hdr_len"] + frames[-1]["plen"] if frames else lead
            if capped:
                dres["consumed"] = frames[-1]["hdr_off"]
            elif parse_status:
                dres["err_off"] = dres["consumed"] = pos
            elif pos > n:
                dres.update(carry_unread=pos - n, consumed=n)
            elif pos < n:
                dres.update(carry_hdr_len=n - pos, consumed=pos)
            else:
                dres["consumed"] = n
        over_frames = capped or len(frames) > cap
        dres.update(status=parse_status or (_lib.FWS_ERR_CAPACITY if over_frames else 0), n_frames=len(frames),
                    n_survivors=len(frames))
        taken = frames[:min(cap, MAX_FRAMES)]
        for i, f in enumerate(taken):
            po = f["hdr_off"] + f["hdr_len"]
            end = po + f["plen"]
            if f["op"] >= 8:
                if not f["fin"] or f["plen"] > 125:
                    err_frame, err_status, resume = i, _lib.FWS_ERR_CONTROL_FRAME, f["hdr_off"]
                    break
                if f["trunc"]:                        # control frames wait whole
                    resume = f["hdr_off"]
                    break
                p = unmask_with(wire[po:end], int.from_bytes(bytes(f["key"]), "little"))
                entries.append(dict(off=len(ctl), len=len(p), first_frame=i, last_frame=i, n_data_frames=1,
                                    opcode=f["op"], utf8_ok=0, flags=0, pad=0))
                units.append((f["op"], p, 0, 1))
                ctl += p
                resume = end
                continue
            if (f["op"] == 0) != is_open:
                err_frame, err_status, resume = i, _lib.FWS_ERR_SEQUENCE, f["hdr_off"]
                break
            if f["op"]:
                is_open, opcode, continued, first, start, nfrag = True, f["op"], False, i, len(dst), 0
                body, total_frames, bad = bytearray(), 0, 0
            elif first == NONE:
                first = i
            key = int.from_bytes(bytes(f["key"]), "little")
            p = unmask_with(wire[po:min(end, n)], key)
            add(p)
            n_data, nfrag, total_frames = n_data + 1, nfrag + 1, total_frames + 1
            if f["trunc"]:                            # taken as far as it is here
                resume = n
                new_frame = dict(frame_unread=end - n, frame_len=f["plen"], frame_key=rotr(key, 8 * (len(p) & 3)),
                                 frame_fin=f["fin"])
                break
            resume = end
            if f["fin"]:
                complete(i)
        deny = len(entries) > msg_cap or len(dst) > dst_cap or len(ctl) > ctl_cap
        status = err_status or dres["status"] or (_lib.FWS_ERR_CAPACITY if deny else 0)
        res = dict(status=status, n_msgs=len(entries), err_frame=err_frame,
                   open_first_frame=first if is_open else NONE, open_opcode=opcode if is_open else 0,
                   n_data_frames=n_data, data_bytes=len(dst), ctl_bytes=len(ctl),
                   open_off=start if is_open else 0, open_len=len(dst) - start if is_open else 0,
                   resume_off=0 if deny else resume)
        text_open = is_open and opcode == TEXT
        msg = dict(open_opcode=opcode if is_open else 0, open_frames=total_frames if is_open else 0,
                   open_bytes=len(body) if is_open else 0, utf8_tail=cc.tail_word(body) if text_open else 0,
                   utf8_bad=bad if text_open else 0, prev_open_opcode=c["open_opcode"],
                   prev_open_frames=c["open_frames"], prev_open_bytes=c["open_bytes"],
                   wire_bytes=c["wire_bytes"] + resume, n_msgs=c["n_msgs"] + len(entries), reserved=0)
        new = dict(new_frame, msg=msg)
        if deny:                                      # nothing delivered: the same bytes come again
            for e in entries:
                e["utf8_ok"] = 0
            dst, ctl, units, new = b"", b"", [], dict(st, msg=dict(c))
        else:
            self.state, self.body = new, bytes(body) if is_open else b""
        recs = np.zeros(min(len(frames), cap, MAX_FRAMES), dtype=_lib.FRAME_INFO)
        for i in range(len(recs)):
            f = frames[i]
            recs[i] = (f["hdr_off"], f["plen"], int.from_bytes(bytes(f["key"]), "little"), f["op"], f["fin"],
                       f["hdr_len"], 1 if f["trunc"] else 0)
        return dict(dst=bytes(dst), ctl=bytes(ctl), entries=entries, units=units, res=res, dres=dres,
                    frames=recs.tobytes(), state=new, n_frames=len(frames))


def feed(ref, stream, cuts, on_call=None, **caps):
    """The stream cut at `cuts` through ref: every call gets the bytes from the
    last resume_off up to the next cut. Returns (units, calls)."""
    pos, units, calls = 0, [], 0
    for b in sorted(set(cuts)) + [len(stream)]:
        while True:
            out = ref.call(stream[pos:b], **caps)
            calls += 1
            if on_call:
                on_call(stream[pos:b], out)
            pos += out["res"]["resume_off"]
            units += out["units"]
            # the header limit: the rest of the same bytes
            if not (out["res"]["status"] == _lib.FWS_ERR_CAPACITY and out["res"]["resume_off"] and pos < b):
                break
        if out["res"]["status"] not in (0, _lib.FWS_ERR_CAPACITY):
            break
    return units, calls
