"""CPU: the ABI surface of fws_gpu_join_messages -- the symbol, the layout of
its three structs against the header and the numpy mirrors, the argument checks
that come before any device call -- and JoinRef (join_ref.py), the GPU tests'
predictor, against FlowRef's units: for random streams cut at random bytes and
halves of 16 bytes to 1 MiB, every record reproduces the unit's bytes from the
buffer it names, a message delivered from the store is intact at the end of the
call that delivers it, and the state tracks fws_msg_carry's. No device calls."""
import ctypes as C
import os
import random
import re

import test_gpu_msg_carry as cc
from flashws_amd import _lib, gpu
from join_ref import DROPPED, IN_CTL, IN_DST, IN_STORE, NOWHERE, JoinRef
from msgflow_ref import FlowRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fws_gpu.h")
NAME = "fws_gpu_join_messages"
HALVES = (16, 48, 4096, 1 << 20)


def test_symbol_is_exported_and_bound():
    L = _lib.lib()
    assert hasattr(L, NAME)
    assert NAME in _lib.exported_symbols()
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    assert sig[NAME][0] is C.c_int and len(sig[NAME][1]) == 14
    assert sig[NAME][1][8] is C.c_uint64                # store_stride
    for f in (gpu.join_messages, gpu.read_join_state, gpu.MessageJoiner):
        assert callable(f)
    assert (_lib.FWS_JOIN_IN_DST, _lib.FWS_JOIN_IN_STORE, _lib.FWS_JOIN_IN_CTL, _lib.FWS_JOIN_NOWHERE,
            _lib.FWS_JOIN_DROPPED) == (0, 1, 2, 3, 1)
    src = open(HEADER).read()
    for name, v in (("IN_DST", 0), ("IN_STORE", 1), ("IN_CTL", 2), ("NOWHERE", 3), ("DROPPED", 1)):
        assert re.search(rf"#define\s+FWS_JOIN_{name}\s+{v}u\b", src), name


def header_fields(src, struct):
    body = re.search(r"typedef struct %s \{(.*?)\}" % struct, src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for typ, names in re.findall(r"\b(u?int\d+_t)\s+([a-z0-9_, ]+);", body):
        out += [(typ, n.strip()) for n in names.split(",")]
    return out


def test_the_three_structs_match_the_header():
    src = open(HEADER).read()
    sizes = dict(re.findall(r"\}\s*(fws_[a-z_]+);\s*/\*\s*(\d+) bytes", src))
    for struct, dt in (("fws_join_state", _lib.JOIN_STATE), ("fws_join_info", _lib.JOIN_INFO),
                       ("fws_join_result", _lib.JOIN_RESULT)):
        assert int(sizes[struct]) == dt.itemsize == 32, struct
        decl = header_fields(src, struct)
        assert [n for _, n in decl] == list(dt.names), struct
        off = 0
        for typ, name in decl:
            w = int(re.search(r"\d+", typ).group()) // 8
            assert dt.fields[name][1] == off and dt.fields[name][0].itemsize == w, (struct, name)
            assert (dt.fields[name][0].kind == "i") == typ.startswith("int"), (struct, name)
            off += w
        assert off == 32, struct


def test_existing_structs_and_the_abi_version_did_not_move():
    src = open(HEADER).read()
    sizes = {k: int(v) for k, v in re.findall(r"\}\s*(fws_[a-z_]+);\s*/\*\s*(\d+) bytes", src)}
    assert (sizes["fws_frame_desc"], sizes["fws_frame_info"], sizes["fws_decode_result"]) == (24, 24, 40)
    assert (sizes["fws_msg_info"], sizes["fws_msg_result"], sizes["fws_msg_carry"], sizes["fws_msg_read"]) == \
        (32, 64, 64, 64)
    assert (sizes["fws_msg_flow"], sizes["fws_reply_state"], sizes["fws_reply_region"]) == (96, 16, 32)
    assert (_lib.MSG_INFO.itemsize, _lib.MSG_RESULT.itemsize, _lib.MSG_READ.itemsize, _lib.MSG_FLOW.itemsize) == \
        (32, 64, 64, 96)
    assert (_lib.REPLY_STATE.itemsize, _lib.REPLY_REGION.itemsize, _lib.TX_RESULT.itemsize) == (16, 32, 32)
    assert re.search(r"#define\s+FWS_GPU_ABI_VERSION\s+1\b", src)
    assert _lib.lib().fws_gpu_abi_version() == 1


def stand_ins():
    """Pointers the checks must never follow: addresses inside one host page pair."""
    page = (C.c_uint8 * 8192)()
    base = (C.addressof(page) + 4095) & ~4095
    ctx, dst, store = base, base + 1024, base + 2048
    reads, msgs, mres, joined, res, states = (base + 4096 + 96 * i for i in range(6))
    ok = [ctx, reads, 4, 4096, msgs, dst, mres, store, 64, joined, res, states, 4, None]
    return page, ok


INDEX = {"ctx": 0, "reads": 1, "n": 2, "max_len": 3, "msgs": 4, "dst": 5, "mres": 6, "store": 7, "stride": 8,
         "joined": 9, "res": 10, "states": 11, "n_conns": 12}


def test_invalid_arguments_fail_before_any_device_call():
    f = getattr(_lib.lib(), NAME)
    page, ok = stand_ins()

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[INDEX[k]] = v
        return f(*a)

    for k in ("ctx", "reads", "msgs", "dst", "mres", "store", "joined", "res", "states"):
        assert call(**{k: None}) == _lib.FWS_ERR_INVALID, k
    assert call(dst=ok[5] + 8) == _lib.FWS_ERR_INVALID
    assert call(store=ok[7] + 4) == _lib.FWS_ERR_INVALID
    for max_len in (0, _lib.FWS_MSG_MULTI_MAX_READ + 1, 0xFFFFFFFF):
        assert call(max_len=max_len) == _lib.FWS_ERR_INVALID, max_len
    for stride in (0, 16, 31, 33, 48, 80, (1 << 32) + 16):
        assert call(stride=stride) == _lib.FWS_ERR_INVALID, stride
    del page


def test_no_reads_is_no_launch():
    f = getattr(_lib.lib(), NAME)
    page, ok = stand_ins()
    a = list(ok)
    a[INDEX["n"]] = 0
    assert f(*a) == 0
    # nothing is looked at with n == 0, not even the arguments that would be refused
    assert f(None, None, 0, 0, None, None, None, None, 0, None, None, None, 0, None) == 0
    del page


def cut_calls(seed, salt=0):
    """FlowRef's outputs for cc.random_stream(seed) cut at random bytes, one call per cut (and per retry)."""
    wire, _, _ = cc.random_stream(seed)
    rng = random.Random(9000 + 31 * salt + seed)
    cuts = sorted({rng.randint(1, len(wire) - 1) for _ in range(rng.randint(3, 12))})
    ref, pos, outs = FlowRef(), 0, []
    for b in cuts + [len(wire)]:
        out = ref.call(wire[pos:b])
        assert out["res"]["status"] == 0, seed
        pos += out["res"]["resume_off"]
        outs.append((out, dict(ref.state["msg"])))
    return outs


def test_joinref_reproduces_the_units_of_flowref():
    stores = drops = both = 0
    for seed in range(40):
        for h, H in enumerate(HALVES):
            outs = cut_calls(seed, h)
            join = JoinRef(H, fill=0xA5)
            for out, carry in outs:
                before = bytes(join.slot)
                got = join.call(out)
                assert got["res"]["status"] == 0 and got["res"]["n_joined"] == len(out["entries"]), (seed, H)
                for rec, e, unit in zip(got["records"], out["entries"], out["units"]):
                    op, body, ok, _ = unit
                    assert (rec["opcode"], rec["utf8_ok"]) == (op, ok)
                    if rec["where"] == IN_CTL:
                        assert op >= 8 and out["ctl"][rec["off"]:rec["off"] + rec["len"]] == body
                    elif rec["where"] == IN_DST:
                        assert not e["flags"] and out["dst"][rec["off"]:rec["off"] + rec["len"]] == body
                    elif rec["where"] == IN_STORE:
                        # at the end of the call: behind the read's open part, which went to the other half
                        assert e["flags"] and join.stored(rec) == body and len(body) <= H, (seed, H)
                        assert rec["off"] in (0, H)
                        stores += 1
                        both += out["res"]["open_opcode"] != 0
                    else:
                        assert rec["where"] == NOWHERE and rec["flags"] == DROPPED and e["flags"]
                        assert rec["len"] == len(body) > H and rec["off"] == 0
                        drops += 1
                st = join.state
                assert (st["open_opcode"], st["open_bytes"]) == (carry["open_opcode"], carry["open_bytes"]), (seed, H)
                assert st["fill"] == (0 if st["dropped"] else st["open_bytes"]) and st["half"] in (0, 1)
                assert st["dropped"] == int(st["open_bytes"] > H)
                assert got["res"]["open_opcode"] == st["open_opcode"] and got["res"]["dropped"] == st["dropped"]
                # only appended ranges changed: the bytes written are exactly `copied`
                changed = sum(a != b for a, b in zip(before, join.slot)) if H <= 4096 else None
                assert changed is None or changed <= got["res"]["copied"]
            assert join.state["open_opcode"] == 0
    assert stores > 100 and drops > 100 and both > 50, (stores, drops, both)


def test_joinref_refuses_what_is_out_of_step():
    body = b"x" * 40
    entry = dict(off=0, len=40, first_frame=0, last_frame=0, n_data_frames=1, opcode=2, utf8_ok=0, flags=0, pad=0)
    res = dict(status=0, n_msgs=1, open_opcode=0, data_bytes=40, ctl_bytes=0, open_off=0, open_len=0)
    whole = dict(res=res, entries=[entry], dst=body, ctl=b"")
    cont = dict(whole, entries=[dict(entry, flags=1)])
    opened = dict(res=dict(res, n_msgs=0, open_opcode=2, open_len=40), entries=[], dst=body, ctl=b"")

    def fresh(open_first):
        j = JoinRef(96, fill=7)
        if open_first:
            assert j.call(opened)["res"] == dict(status=0, n_joined=0, copied=40, open_opcode=2, dropped=0, reserved=0)
        return j

    for open_first, out in ((False, cont),                                   # a CONTINUED entry, nothing open
                            (True, dict(cont, entries=[entry, dict(entry, flags=1)], res=dict(res, n_msgs=2))),
                            (True, whole),                                   # a data entry, a message open
                            (True, dict(opened, res=dict(opened["res"], open_opcode=1))),
                            (True, dict(opened, res=dict(opened["res"], open_opcode=0))),
                            (False, dict(whole, entries=[dict(entry, len=(128 << 10) + 1)])),
                            (False, dict(opened, res=dict(opened["res"], open_len=(128 << 10) + 1))),
                            (False, dict(whole, res=dict(res, n_msgs=258), entries=[entry] * 258))):
        j = fresh(open_first)
        state, slot = dict(j.state), bytes(j.slot)
        got = j.call(out)
        assert got["res"]["status"] == _lib.FWS_ERR_INVALID and not got["records"], out["res"]
        assert got["res"] == dict(status=_lib.FWS_ERR_INVALID, n_joined=0, copied=0, open_opcode=0, dropped=0,
                                  reserved=0)
        assert j.state == state and bytes(j.slot) == slot
    # an undelivered decode and a declined read: nothing to do, the state echoed
    j = fresh(True)
    state, slot = dict(j.state), bytes(j.slot)
    for out, caps in ((whole, dict(dst_cap=39)), (whole, dict(msg_cap=0)),
                      (dict(whole, res=dict(res, ctl_bytes=5)), dict(ctl_cap=4)),
                      (dict(whole, res=dict(res, status=_lib.FWS_ERR_DECLINED)), {})):
        got = j.call(out, **caps)
        assert got == dict(res=dict(status=0, n_joined=0, copied=0, open_opcode=2, dropped=0, reserved=0), records=[])
        assert j.state == state and bytes(j.slot) == slot
    # in step again: the message completes from the store
    got = j.call(cont)
    assert got["records"][0]["where"] == IN_STORE and j.stored(got["records"][0]) == body + body
