"""CPU: the ABI surface of fws_gpu_publish_messages -- the symbol, fws_pub_sub and
the constants against the header and the numpy mirror, the argument checks that
come before any device call -- and publish_ref, the GPU tests' predictor: its
bytes for single-item lists against txmulti_ref (which test_tx_multi_cpu.py holds
against the reference's recorded frames), a list's bytes against its items', and
the order of the refusals. No device calls."""
import ctypes as C
import os
import random
import re

import numpy as np

import publish_ref as pr
import txmulti_ref as tr
from flashws_amd import _lib, gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fws_gpu.h")
NAME = "fws_gpu_publish_messages"


def test_symbol_is_exported_and_bound():
    L = _lib.lib()
    assert hasattr(L, NAME) and NAME in _lib.exported_symbols()
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    assert sig[NAME][0] is C.c_int and len(sig[NAME][1]) == 18
    for i in (2, 7, 9, 10, 16):                          # n_msgs, n_list, n, max_len, n_conns
        assert sig[NAME][1][i] is C.c_uint32, i
    assert callable(gpu.publish_messages) and callable(gpu.MessagePublisher)


def header_fields(src, struct):
    body = re.search(r"typedef struct %s \{(.*?)\}" % struct, src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for typ, names in re.findall(r"\b(u?int\d+_t)\s+([a-z0-9_, ]+);", body):
        out += [(typ, n.strip()) for n in names.split(",")]
    return out


def test_pub_sub_is_32_bytes_in_the_header_order():
    src = open(HEADER).read()
    sizes = {k: int(v) for k, v in re.findall(r"\}\s*(fws_[a-z_]+);\s*/\*\s*(\d+) bytes", src)}
    assert sizes["fws_pub_sub"] == _lib.PUB_SUB.itemsize == 32
    decl = header_fields(src, "fws_pub_sub")
    assert [n for _, n in decl] == list(_lib.PUB_SUB.names) == ["out_off", "out_cap", "conn", "list_off", "list_len",
                                                                 "frame_base", "frame_cap"]
    off = 0
    for typ, name in decl:
        w = int(re.search(r"\d+", typ).group()) // 8
        assert _lib.PUB_SUB.fields[name][1] == off and _lib.PUB_SUB.fields[name][0].itemsize == w, name
        assert _lib.PUB_SUB.fields[name][0].kind == "u" and typ.startswith("uint"), name
        off += w
    assert off == 32
    assert re.search(r"#define\s+FWS_PUB_MAX_ITEMS\s+256u\b", src) and _lib.FWS_PUB_MAX_ITEMS == 256
    # the structs it stands beside did not move
    assert (sizes["fws_join_info"], sizes["fws_tx_result"], sizes["fws_tx_conn"], sizes["fws_reply_state"],
            sizes["fws_frame_info"]) == (32, 32, 32, 16, 24)
    assert re.search(r"#define\s+FWS_GPU_ABI_VERSION\s+1\b", src) and _lib.lib().fws_gpu_abi_version() == 1


def stand_ins():
    """Pointers the checks must never follow: addresses inside one host page pair."""
    page = (C.c_uint8 * 8192)()
    base = (C.addressof(page) + 4095) & ~4095
    ctx, out, dst, store, ctl = base, base + 1024, base + 2048, base + 2048 + 256, base + 2048 + 512
    msgs, lst, subs, frames, res, conns, states = (base + 4096 + 96 * i for i in range(7))
    ok = [ctx, msgs, 4, dst, store, ctl, lst, 4, subs, 4, 4096, out, frames, res, conns, states, 4, None]
    return page, ok


INDEX = {"ctx": 0, "msgs": 1, "n_msgs": 2, "dst": 3, "store": 4, "ctl": 5, "list": 6, "n_list": 7, "subs": 8, "n": 9,
         "max_len": 10, "out": 11, "frames": 12, "res": 13, "conns": 14, "states": 15, "n_conns": 16}


def test_invalid_arguments_fail_before_any_device_call():
    f = getattr(_lib.lib(), NAME)
    page, ok = stand_ins()

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[INDEX[k]] = v
        return f(*a)

    for k in ("ctx", "msgs", "list", "subs", "out", "res", "conns", "states"):
        assert call(**{k: None}) == _lib.FWS_ERR_INVALID, k
    for d in (1, 4, 8):
        assert call(out=ok[INDEX["out"]] + d) == _lib.FWS_ERR_INVALID, d
    for max_len in (0, _lib.FWS_TX_MULTI_MAX_SEND + 1, 0xFFFFFFFF):
        assert call(max_len=max_len) == _lib.FWS_ERR_INVALID, max_len
    # the optional pointers do not rescue a refused call
    assert call(dst=None, store=None, ctl=None, frames=None, max_len=0) == _lib.FWS_ERR_INVALID
    del page


def test_no_subscribers_is_no_launch():
    f = getattr(_lib.lib(), NAME)
    page, ok = stand_ins()
    a = list(ok)
    a[INDEX["n"]] = 0
    assert f(*a) == 0
    # nothing is looked at with n == 0, not even the arguments that would be refused
    assert f(None, None, 0, None, None, None, None, 0, None, 0, 0, None, None, None, None, None, 0, None) == 0
    del page


LENS = (0, 1, 2, 3, 13, 14, 15, 16, 17, 124, 125, 126, 127, 4096, 65535, 65536, 65537, 128 << 10)


def buffers(seed, total=3 * (128 << 10) + 4096):
    rng = np.random.default_rng(seed)
    return tuple(rng.integers(0, 256, total, dtype=np.uint8).tobytes() for _ in range(3))


def test_single_item_lists_equal_the_encode_model():
    """One record, one frame: what fws_gpu_encode_messages_multi's model gives for the same payload as an
    unmasked whole send -- that model replays the reference's recorded SendFrame bytes."""
    bases = buffers(1)
    rng = random.Random(2)
    n = 0
    for ln in LENS:
        for op in (pr.TEXT, pr.BIN, pr.CLOSE, pr.PING, pr.PONG):
            if op >= 8 and ln > 125:
                continue
            where, off = rng.randrange(3), rng.randrange(0, 4096)
            recs = pr.records([(op, where, off, ln)])
            tx = dict(pr.new_tx(), frames=rng.randrange(9), wire_bytes=rng.randrange(1 << 20))
            got = pr.predict(tx, pr.new_state(), recs, bases, [0])
            want = tr.predict(tx, bases[where][off:off + ln], op, 1, masked=False, max_frame=0)
            assert got["res"] == want["res"] and got["bytes"] == want["bytes"], (ln, op)
            assert got["records"].tobytes() == want["records"].tobytes() and got["tx"] == want["state"], (ln, op)
            assert got["state"]["close_sent"] == int(op == pr.CLOSE)
            assert got["frames"] == [(op, 1, bases[where][off:off + ln])]
            n += 1
    assert n == 5 * 11 + 2 * 7


def test_a_list_is_the_concatenation_of_its_items():
    bases = buffers(3)
    rng = random.Random(4)
    for trial in range(120):
        k = rng.choice([1, 2, 3, 7, 40])
        items = []
        for _ in range(k):
            op = rng.choice([1, 2, 2, 9, 10, 0])
            ln = rng.choice(LENS[:11]) if op >= 8 else rng.choice(LENS[:15])
            where = rng.choice([0, 1, 2, 3]) if op else rng.randrange(256)
            items.append((op, where, rng.randrange(0, 5000), ln))
        recs = pr.records(items)
        lst = [rng.randrange(k) for _ in range(rng.randrange(0, 2 * k + 1))]   # any order, repeats allowed
        tx, st = dict(pr.new_tx(), frames=5, wire_bytes=999), pr.new_state()
        whole = pr.predict(tx, st, recs, bases, lst)
        assert whole["res"]["status"] == 0, trial
        wire, recs_out, frames, cur = b"", [], [], tx
        for i in lst:
            one = pr.predict(cur, st, recs, bases, [i])
            assert one["res"]["status"] == 0 and one["res"]["n_frames"] == (0 if pr.is_nothing(recs[i]) else 1)
            for r in one["records"]:
                r = r.copy()
                r["hdr_off"] = len(wire)
                recs_out.append(r)
            wire += one["bytes"]
            frames += one["frames"]
            cur = one["tx"]
        assert whole["bytes"] == wire and whole["frames"] == frames and whole["tx"] == cur, trial
        assert whole["records"].tobytes() == np.array(recs_out, dtype=_lib.FRAME_INFO).tobytes()
        assert whole["res"] == dict(status=0, n_frames=len(frames), out_len=len(wire), last_msg_not_fin=0, pad=0,
                                    reserved=0)
        assert whole["state"] is st


def test_close_drops_what_follows_and_sets_close_sent():
    bases = buffers(5)
    recs = pr.records([(2, 0, 0, 10), (8, 2, 3, 2), (1, 1, 7, 20), (9, 2, 0, 4)])
    st = dict(pr.new_state(), close_code=1000, fail_code=1002)
    got = pr.predict(pr.new_tx(), st, recs, bases, [0, 3, 1, 2, 0, 1])
    assert [f[0] for f in got["frames"]] == [2, 9, 8] and got["res"]["n_frames"] == 3
    assert got["state"] == dict(st, close_sent=1)        # close_code and fail_code stay what they were
    assert got["bytes"] == b"".join(pr.predict(pr.new_tx(), st, recs, bases, [i])["bytes"] for i in (0, 3, 1))
    # and the next call says nothing
    again = pr.predict(got["tx"], got["state"], recs, bases, [0])
    assert again["res"] == dict(tr.refusal(0), last_msg_not_fin=0) and again["tx"] is got["tx"]


def test_refusals_and_their_order():
    """One case per adjacent pair of rows: with both causes present the earlier row is the verdict, and with
    the earlier cause taken away the later one."""
    bases = buffers(6)
    big = (128 << 10) + 1
    # 0 data, 1 PING, 2 over-long PING, 3 over-long data, 4 CLOSE, 5 bad opcode, 6 nothing, 7 where above 3
    recs = pr.records([(2, 0, 0, 100), (9, 2, 0, 5), (9, 2, 0, 126), (1, 1, 0, big), (8, 2, 0, 2), (3, 0, 0, 1),
                       (0, 9, 0, 0), (2, 4, 0, 1)])
    tx, st = pr.new_tx(), pr.new_state()
    open_tx, closed = dict(tx, last_msg_not_fin=1), dict(st, close_sent=1)

    def status(lst, tx=tx, st=st, **kw):
        got = pr.predict(tx, st, recs, bases, lst, **kw)
        if got["res"]["status"]:
            assert got["bytes"] == b"" and got["tx"] is tx and got["state"] is st and len(got["records"]) == 0
            if got["res"]["status"] != pr.CAPACITY:
                assert got["res"] == tr.refusal(got["res"]["status"])
        return got["res"]["status"]

    # row 1, each cause alone
    assert status([0], out_off=8) == status([0], conn_ok=False) == status([0], list_ok=False) == pr.INVALID
    assert status([0] * 257) == pr.INVALID and status([0] * 256) == 0
    assert status([0, 8]) == status([5]) == status([7]) == pr.INVALID
    assert pr.predict(tx, st, recs, (None, bases[1], bases[2]), [1, 0])["res"]["status"] == pr.INVALID
    assert pr.predict(tx, st, recs, (None, bases[1], bases[2]), [1])["res"]["status"] == 0
    # 1 before 2: close_sent does not hide an invalid list; without the invalid item, no frames
    assert status([0, 5], st=closed) == pr.INVALID and status([0], st=closed) == 0
    got = pr.predict(open_tx, closed, recs, bases, [0])
    assert got["res"] == dict(tr.refusal(0), last_msg_not_fin=1) and got["tx"] is open_tx
    assert pr.predict(open_tx, st, recs, bases, [6, 6])["res"] == dict(tr.refusal(0), last_msg_not_fin=1)
    assert pr.predict(open_tx, st, recs, bases, [])["res"] == dict(tr.refusal(0), last_msg_not_fin=1)
    # 2 before 3: close_sent hides an over-long control record
    assert status([2], st=closed) == 0 and status([2]) == pr.CONTROL
    # 3 before 4; both are judged behind a CLOSE as well
    assert status([3, 2]) == pr.CONTROL and status([3]) == pr.DECLINED
    assert status([4, 2]) == pr.CONTROL and status([4, 3]) == pr.DECLINED
    assert status([0], max_len=99) == pr.DECLINED and status([0], max_len=100) == 0
    # 4 before 5
    assert status([0, 3], tx=open_tx) == pr.DECLINED and status([0], tx=open_tx) == pr.SEQUENCE
    # 5 before 6
    assert status([0], tx=open_tx, out_cap=1) == pr.SEQUENCE and status([0], out_cap=101) == pr.CAPACITY
    assert pr.predict(tx, st, recs, bases, [0, 1], out_cap=108)["res"] == tr.refusal(pr.CAPACITY, 2, 109)
    assert status([0, 1], out_cap=109) == 0
    # control frames go through an open message and leave it open; so does data behind a CLOSE
    for lst, n in (([1, 1], 2), ([1, 4, 0], 2), ([4, 0, 0], 1)):
        got = pr.predict(open_tx, st, recs, bases, lst)
        assert got["res"]["status"] == 0 and got["res"]["n_frames"] == n and got["res"]["last_msg_not_fin"] == 1
        assert got["tx"]["last_msg_not_fin"] == 1 and got["tx"]["frames"] == n
    assert status([1, 0, 4], tx=open_tx) == pr.SEQUENCE
    # records are shown up to frame_cap; more frames than that is no error
    got = pr.predict(tx, st, recs, bases, [0, 1, 0], frame_cap=2)
    assert got["res"]["n_frames"] == 3 and len(got["records"]) == 2
