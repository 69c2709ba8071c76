"""CPU: the ABI surface of fws_gpu_decode_messages_flow -- the symbol, the layout
of fws_msg_flow against the header and the numpy mirror, the argument checks
that come before any device call -- and FlowRef (msgflow_ref.py), the GPU
tests' predictor, against the oracle's OnRecvData: for valid random streams cut
at random bytes the parts FlowRef delivers, joined per message, and the order
of units are what the session hands out read by read, and after every read a
data frame in progress has the session's unread_pl_len and rotated key. No
device calls."""
import ctypes as C
import os
import random
import re

import orc
import test_gpu_msg_carry as cc
from flashws_amd import _lib, gpu
from msgflow_ref import FlowRef, feed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fws_gpu.h")
NAME = "fws_gpu_decode_messages_flow"


def test_symbol_is_exported_and_bound():
    L = _lib.lib()
    assert hasattr(L, NAME)
    assert NAME in _lib.exported_symbols()
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    assert sig[NAME] == sig["fws_gpu_decode_messages_multi"]      # the same arguments, the state for the carry
    assert sig[NAME][0] is C.c_int and len(sig[NAME][1]) == 14
    assert callable(gpu.decode_messages_flow) and callable(gpu.MessageFlow)


def test_flow_state_is_96_bytes_in_the_header_order_with_msg_first():
    src = open(HEADER).read()
    sizes = dict(re.findall(r"\}\s*(fws_[a-z_]+);\s*/\*\s*(\d+) bytes", src))
    assert int(sizes["fws_msg_flow"]) == _lib.MSG_FLOW.itemsize == 96
    body = re.search(r"typedef struct fws_msg_flow \{(.*?)\}", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = re.findall(r"\b(fws_msg_carry|u?int\d+_t)\s+([a-z0-9_]+)(?:\[(\d+)\])?\s*;", body)
    assert [d[1] for d in decl] == ["msg", "frame_unread", "frame_len", "frame_key", "frame_fin", "pad", "reserved"]
    dt = _lib.MSG_FLOW
    assert list(dt.names) == [d[1] for d in decl]
    assert dt.fields["msg"][0] == _lib.MSG_CARRY and dt.fields["msg"][1] == 0
    off = 0
    for typ, name, count in decl:
        w = 64 if typ == "fws_msg_carry" else int(re.search(r"\d+", typ).group()) // 8 * int(count or 1)
        assert dt.fields[name][1] == off and dt.fields[name][0].itemsize == w, name
        off += w
    assert off == 96
    assert _lib.FWS_MSG_FLOW_MAX_PENDING == 138


def test_existing_structs_and_the_abi_version_did_not_move():
    src = open(HEADER).read()
    sizes = {k: int(v) for k, v in re.findall(r"\}\s*(fws_[a-z_]+);\s*/\*\s*(\d+) bytes", src)}
    assert (sizes["fws_frame_desc"], sizes["fws_frame_info"], sizes["fws_decode_result"]) == (24, 24, 40)
    assert (sizes["fws_msg_info"], sizes["fws_msg_result"], sizes["fws_msg_carry"], sizes["fws_msg_read"]) == \
        (32, 64, 64, 64)
    assert (_lib.FRAME_INFO.itemsize, _lib.DECODE_RESULT.itemsize, _lib.MSG_READ.itemsize) == (24, 40, 64)
    assert (_lib.MSG_INFO.itemsize, _lib.MSG_RESULT.itemsize, _lib.MSG_CARRY.itemsize) == (32, 64, 64)
    assert re.search(r"#define\s+FWS_GPU_ABI_VERSION\s+1\b", src)
    assert _lib.lib().fws_gpu_abi_version() == 1
    assert _lib.FWS_MSG_MULTI_MAX_READ == 128 << 10 and _lib.FWS_MSG_MULTI_MAX_FRAMES == 256


def stand_ins():
    """Pointers the checks must never follow: addresses inside one host page pair."""
    page = (C.c_uint8 * 8192)()
    base = (C.addressof(page) + 4095) & ~4095
    ctx, wire, dst = base, base + 1024, base + 2048
    reads, frames, msgs, ctl, res, mres, flows = (base + 4096 + 96 * i for i in range(7))
    ok = [ctx, wire, reads, 4, 4096, frames, msgs, dst, ctl, res, mres, flows, 4, None]
    return page, ok


INDEX = {"ctx": 0, "wire": 1, "reads": 2, "n": 3, "max_len": 4, "frames": 5, "msgs": 6, "dst": 7, "ctl": 8, "res": 9,
         "mres": 10, "flows": 11, "n_conns": 12}


def test_invalid_arguments_fail_before_any_device_call():
    f = getattr(_lib.lib(), NAME)
    page, ok = stand_ins()

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[INDEX[k]] = v
        return f(*a)

    for k in ("ctx", "wire", "reads", "frames", "msgs", "dst", "ctl", "res", "mres", "flows"):
        assert call(**{k: None}) == _lib.FWS_ERR_INVALID, k
    assert call(wire=ok[1] + 4) == _lib.FWS_ERR_INVALID
    assert call(dst=ok[7] + 8) == _lib.FWS_ERR_INVALID
    assert call(max_len=0) == _lib.FWS_ERR_INVALID
    assert call(max_len=_lib.FWS_MSG_MULTI_MAX_READ + 1) == _lib.FWS_ERR_INVALID
    assert call(max_len=0xFFFFFFFF) == _lib.FWS_ERR_INVALID
    del page


def test_no_reads_is_no_launch():
    f = getattr(_lib.lib(), NAME)
    page, ok = stand_ins()
    a = list(ok)
    a[INDEX["n"]] = 0
    assert f(*a) == 0
    # nothing is looked at with n == 0, not even the arguments that would be refused
    assert f(*([None] * 3 + [0, 0] + [None] * 7 + [0, None])) == 0
    del page


def session_units(session, data, open_parts, units, pong_parts):
    """One read through the oracle's OnRecvData: completed units appended to units."""
    ret, buf, ev, ctl = session.feed(data)
    assert ret == 0
    for e in ev:
        kind = int(e["kind"])
        if kind == 0 and not e["is_ctl"]:             # ON_READ: a data part
            o = int(e["data_off"])
            open_parts.append(buf[o:o + int(e["size"])].tobytes())
            if e["msg_end"]:
                units.append((int(e["opcode"]), b"".join(open_parts)))
                open_parts.clear()
        elif kind == 0:                               # a PONG is handed out as it arrives, like data
            o = int(e["ctl_off"])
            pong_parts.append(ctl[o:o + int(e["size"])].tobytes())
            if e["frame_end"]:
                units.append((cc.PONG, b"".join(pong_parts)))
                pong_parts.clear()
        elif kind in (1, 2):                          # PING answered, CLOSE: whole
            o = int(e["ctl_off"])
            units.append((cc.PING if kind == 1 else cc.CLOSE, ctl[o:o + int(e["size"])].tobytes()))


def test_flowref_delivers_what_the_oracle_session_delivers():
    in_progress = 0
    for seed in range(40):
        wire, _, _ = cc.random_stream(seed)
        rng = random.Random(7000 + seed)
        cuts = sorted({rng.randint(1, len(wire) - 1) for _ in range(rng.randint(3, 12))})
        session, ref = orc.OrcSession(is_server=True), FlowRef()
        want, got, open_parts, parts, pong_parts = [], [], [], [], []
        pos = last = 0
        for b in cuts + [len(wire)]:
            session_units(session, wire[last:b], open_parts, want, pong_parts)
            last = b
            out = ref.call(wire[pos:b])
            assert out["res"]["status"] == 0, seed
            pos += out["res"]["resume_off"]
            assert b - pos <= _lib.FWS_MSG_FLOW_MAX_PENDING
            # the call's parts joined per message, the units in their order
            for e in out["entries"]:
                if e["opcode"] >= 8:
                    got.append((e["opcode"], out["ctl"][e["off"]:e["off"] + e["len"]]))
                    continue
                body = out["dst"][e["off"]:e["off"] + e["len"]]
                if e["flags"] & _lib.FWS_MSG_CONTINUED:
                    body = b"".join(parts) + body
                parts = []
                got.append((e["opcode"], body))
            if out["res"]["open_opcode"] and out["res"]["open_len"]:
                o = out["res"]["open_off"]
                parts.append(out["dst"][o:o + out["res"]["open_len"]])
            assert got == want[:len(got)], (seed, b)
            msg = ref.state["msg"]                    # FlowRef keeps utf8_bad up as bytes arrive: the walk's rule
            text_open = msg["open_opcode"] == cc.TEXT
            assert msg["utf8_bad"] == (cc.prefix_bad(ref.body) if text_open else 0), (seed, b)
            assert msg["utf8_tail"] == (cc.tail_word(ref.body) if text_open else 0)
            if ref.state["frame_unread"]:
                head = session.head()
                assert head.unread_pl_len == ref.state["frame_unread"], (seed, b)
                assert head.last_rx_mask_key == ref.state["frame_key"], (seed, b)
                assert head.last_rx_fin_flag == ref.state["frame_fin"] and pos == b
                in_progress += 1
        assert got == want and pos == len(wire), seed
        assert [(u[0], u[1]) for u in cc.whole(wire)[0]] == want, seed
    assert in_progress > 40


def test_flowref_delivers_the_same_units_for_every_cut():
    stream = cc.twelve_frames()
    units, status, _ = cc.whole(stream)
    assert status == 0 and len(units) == 8
    for cut in range(len(stream) + 1):
        ref = FlowRef()
        got, calls = feed(ref, stream, [cut])
        assert got == units and ref.state["msg"]["wire_bytes"] == len(stream), cut
        assert ref.state["frame_unread"] == 0 and ref.state["msg"]["n_msgs"] == 8


def test_flowref_equals_refconn_on_whole_frames():
    for seed in range(40):
        wire, spans, _ = cc.random_stream(seed)
        a, b = cc.RefConn(), FlowRef()
        for cap in (cc.BIG, 7):
            x, y = a.call(wire, cap=cap), b.call(wire, cap=cap)
            for k in ("dst", "ctl", "entries", "units", "res", "n_frames"):
                assert x[k] == y[k], (seed, cap, k)
            assert y["state"]["msg"] == x["carry"] and y["state"]["frame_unread"] == 0
