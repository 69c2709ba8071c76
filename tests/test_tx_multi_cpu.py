"""CPU: the ABI surface of fws_gpu_encode_messages_multi -- the symbol, the three
structs and constants against the header and the numpy mirror, the argument
checks that come before any device call -- and txmulti_ref, the GPU tests'
predictor, against the reference's recorded SendFrame bytes
(tests/golden/tx_cases.json.gz) and against itself. No device calls."""
import ctypes as C
import os
import random
import re

import numpy as np

import txmulti_ref as tr
from flashws_amd import _lib, gpu
from test_tx_cpu import SESSIONS, frame_matches, tx_payload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fws_gpu.h")
NAME = "fws_gpu_encode_messages_multi"


def test_symbol_is_exported_and_bound():
    L = _lib.lib()
    assert hasattr(L, NAME) and NAME in _lib.exported_symbols()
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    assert sig[NAME][0] is C.c_int and len(sig[NAME][1]) == 11
    assert callable(gpu.encode_messages_multi) and callable(gpu.read_tx_conn) and callable(gpu.MessageSender)


def header_struct(src, name):
    body = re.search(r"typedef struct %s \{(.*?)\}" % name, src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for typ, names in re.findall(r"\b(u?int\d+_t)\s+([a-z0-9_,\[\] ]+);", body):
        for nm in names.split(","):
            m = re.match(r"\s*([a-z0-9_]+)(?:\[(\d+)\])?\s*$", nm)
            out.append((m.group(1), int(re.search(r"\d+", typ).group()) // 8 * int(m.group(2) or 1)))
    return out


def test_structs_are_32_64_32_bytes_in_the_header_order():
    src = open(HEADER).read()
    sizes = {k: int(v) for k, v in re.findall(r"\}\s*(fws_[a-z_]+);\s*/\*\s*(\d+) bytes", src)}
    assert (sizes["fws_tx_conn"], sizes["fws_tx_send"], sizes["fws_tx_result"]) == (32, 64, 32)
    for name, dt, size in (("fws_tx_conn", _lib.TX_CONN, 32), ("fws_tx_send", _lib.TX_SEND, 64),
                           ("fws_tx_result", _lib.TX_RESULT, 32)):
        decl = header_struct(src, name)
        assert [d[0] for d in decl] == list(dt.names), name
        off = 0
        for field, width in decl:
            assert dt.fields[field][1] == off and dt.fields[field][0].itemsize == width, (name, field)
            off += width
        assert off == dt.itemsize == size, name
    # the structs the new ones stand beside did not move
    assert (sizes["fws_tx_desc"], sizes["fws_frame_info"], sizes["fws_msg_read"], sizes["fws_msg_flow"]) == \
        (24, 24, 64, 96)
    assert _lib.lib().fws_gpu_abi_version() == 1


def test_constants_match_the_header():
    src = open(HEADER).read()
    assert re.search(r"#define\s+FWS_TX_MULTI_MAX_SEND\s+\(128u << 10\)", src)
    assert re.search(r"#define\s+FWS_TX_MULTI_MAX_FRAMES\s+256u", src)
    assert re.search(r"#define\s+FWS_TX_FRAG_KEY\(key, j\)\s+\(\(uint32_t\)\(\(key\) \+ \(uint32_t\)\(j\) \* "
                     r"0x9E3779B9u\)\)", src)
    assert _lib.FWS_TX_MULTI_MAX_SEND == 128 << 10 and _lib.FWS_TX_MULTI_MAX_FRAMES == 256
    for key in (0, 1, 0x12345678, 0xFFFFFFFF):
        assert _lib.FWS_TX_FRAG_KEY(key, 0) == key
        assert _lib.FWS_TX_FRAG_KEY(key, 1) == (key + 0x9E3779B9) % (1 << 32)
        assert _lib.FWS_TX_FRAG_KEY(key, 255) == (key + 255 * 0x9E3779B9) % (1 << 32)


def stand_ins():
    """Pointers the checks must never follow: addresses inside one host page pair."""
    page = (C.c_uint8 * 8192)()
    base = (C.addressof(page) + 4095) & ~4095
    ctx, out, src = base, base + 1024, base + 2048
    sends, frames, res, conns = (base + 4096 + 96 * i for i in range(4))
    ok = [ctx, out, src, sends, 4, 4096, frames, res, conns, 4, None]
    return page, ok


INDEX = {"ctx": 0, "out": 1, "src": 2, "sends": 3, "n": 4, "max_len": 5, "frames": 6, "res": 7, "conns": 8,
         "n_conns": 9}


def test_invalid_arguments_fail_before_any_device_call():
    f = getattr(_lib.lib(), NAME)
    page, ok = stand_ins()

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[INDEX[k]] = v
        return f(*a)

    for k in ("ctx", "out", "src", "sends", "res", "conns"):
        assert call(**{k: None}) == _lib.FWS_ERR_INVALID, k
    assert call(out=ok[1] + 4) == _lib.FWS_ERR_INVALID
    assert call(out=ok[1] + 8) == _lib.FWS_ERR_INVALID
    assert call(max_len=0) == _lib.FWS_ERR_INVALID
    assert call(max_len=_lib.FWS_TX_MULTI_MAX_SEND + 1) == _lib.FWS_ERR_INVALID
    assert call(max_len=0xFFFFFFFF) == _lib.FWS_ERR_INVALID
    del page


def test_no_sends_is_no_launch():
    f = getattr(_lib.lib(), NAME)
    page, ok = stand_ins()
    a = list(ok)
    a[INDEX["n"]] = 0
    assert f(*a) == 0
    # nothing is looked at with n == 0, not even the arguments that would be refused
    assert f(*([None] * 4 + [0, 0] + [None] * 3 + [0, None])) == 0
    del page


def test_model_replays_the_reference_sessions_frame_by_frame():
    """Every recorded WriteFrame call as one send with max_frame = 0: the model's
    bytes are the bytes the reference's SendFrame wrote, and the state it carries
    is the session's last_msg_not_fin. The sessions hold frames above
    FWS_TX_MULTI_MAX_SEND (one is 1 MiB): the call declines those, and the model's
    bytes for them are checked with its limit lifted."""
    big = 1 << 32
    over = 0
    for sess in SESSIONS:
        state, masked = tr.new_state(), not sess["server"]
        total = 0
        for i, r in enumerate(sess["frames"]):
            args = (state, tx_payload(r["seed"], r["len"]), r["frame_type"], r["last"])
            out = tr.predict(*args, masked=masked, key=r["key"], max_frame=0)
            if r["len"] > _lib.FWS_TX_MULTI_MAX_SEND:
                assert out["res"] == tr.refusal(tr.DECLINED) and out["state"] is state
                out = tr.predict(*args, masked=masked, key=r["key"], max_frame=0, max_len=big, max_send=big)
                over += 1
            assert out["res"]["status"] == 0 and out["res"]["n_frames"] == 1, i
            assert frame_matches(r, out["bytes"]), (sess["server"], i, r["len"], r["frame_type"], r["last"])
            rec = out["records"][0]
            b0 = int((r.get("hex") or r["head_hex"])[:2], 16)
            assert (int(rec["opcode"]), int(rec["fin"])) == (b0 & 15, b0 >> 7), i
            assert int(rec["key"]) == (r["key"] if masked else 0) and int(rec["payload_len"]) == r["len"]
            assert int(rec["hdr_len"]) == r["size"] - r["len"] and int(rec["hdr_off"]) == 0
            state = out["state"]
            total += r["size"]
            assert state["frames"] == i + 1 and state["wire_bytes"] == total
            assert out["res"]["last_msg_not_fin"] == state["last_msg_not_fin"]
            if not r["frame_type"] & 8:
                assert state["last_msg_not_fin"] == (0 if r["last"] else 1), i
    assert over >= 2


def test_a_fragmented_send_equals_the_single_frame_sends_of_its_slices():
    rng = random.Random(11)
    for trial in range(200):
        m = rng.choice([1, 2, 3, 13, 16, 125, 126, 127, 1000, 4096])
        n = rng.choice([0, 1, m - 1, m, m + 1, 2 * m, 3 * m + 1, 17 * m - 1, rng.randrange(0, 40 * m)])
        n = min(n, 256 * m)
        payload = bytes(rng.getrandbits(8) for _ in range(n))
        masked, last, ft, key = rng.random() < 0.5, rng.random() < 0.5, rng.choice([1, 2]), rng.getrandbits(32)
        start = dict(tr.new_state(), last_msg_not_fin=rng.randrange(2), frames=rng.randrange(9), wire_bytes=77)
        whole = tr.predict(start, payload, ft, last, masked=masked, key=key, max_frame=m)
        cut = tr.slices(n, m)
        assert whole["res"]["status"] == 0 and whole["res"]["n_frames"] == len(cut) == max(1, -(-n // m))
        state, wire, recs = start, b"", []
        for j, (o, ln) in enumerate(cut):
            one = tr.predict(state, payload[o:o + ln], ft, last and j == len(cut) - 1, masked=masked,
                             key=tr.frag_key(key, j), max_frame=0)
            assert one["res"]["n_frames"] == 1
            rec = one["records"][0].copy()
            rec["hdr_off"] = len(wire)
            recs.append(rec)
            wire += one["bytes"]
            state = one["state"]
        assert whole["bytes"] == wire and whole["state"] == state, (trial, n, m)
        assert whole["records"].tobytes() == np.array(recs, dtype=_lib.FRAME_INFO).tobytes()
        assert whole["res"]["out_len"] == len(wire)
        # frames 1.. are continuations, FIN on the last one only, the keys follow FWS_TX_FRAG_KEY
        assert all(int(r["opcode"]) == 0 for r in whole["records"][1:])
        assert [int(r["fin"]) for r in whole["records"]] == [0] * (len(cut) - 1) + [int(last)]
        assert [int(r["key"]) for r in whole["records"]] == [tr.frag_key(key, j) if masked else 0
                                                             for j in range(len(cut))]


def test_model_refusals_and_their_order():
    st = tr.new_state()
    p = b"x" * 200
    assert tr.predict(st, p, 9, 1)["res"] == tr.refusal(tr.CONTROL)
    assert tr.predict(st, p, 3, 1)["res"] == tr.refusal(tr.INVALID)
    assert tr.predict(st, p, 9, 1, out_off=8)["res"] == tr.refusal(tr.INVALID)
    assert tr.predict(st, p, 1, 1, conn_ok=False)["res"] == tr.refusal(tr.INVALID)
    assert tr.predict(st, p, 1, 1, max_len=199)["res"] == tr.refusal(tr.DECLINED)
    assert tr.predict(st, b"x" * 257, 1, 1, max_frame=1)["res"] == tr.refusal(tr.DECLINED)
    assert tr.predict(st, b"x" * 256, 1, 1, max_frame=1)["res"]["n_frames"] == 256
    need = 2 * (8 + 126)
    assert tr.predict(st, b"x" * 252, 1, 1, max_frame=126, out_cap=need - 1)["res"] == \
        tr.refusal(tr.CAPACITY, 2, need)
    ok = tr.predict(st, b"x" * 252, 1, 1, max_frame=126, out_cap=need, frame_cap=1)
    assert ok["res"]["status"] == 0 and ok["res"]["n_frames"] == 2 and len(ok["records"]) == 1
    # a refusal leaves the state object itself
    assert tr.predict(st, p, 9, 1)["state"] is st
    # control frames neither use nor change the state; FIN is `last`
    open_ = dict(st, last_msg_not_fin=1)
    ping = tr.predict(open_, b"hi", 9, 0, max_frame=1)
    assert ping["res"]["n_frames"] == 1 and ping["state"]["last_msg_not_fin"] == 1
    assert (int(ping["records"][0]["opcode"]), int(ping["records"][0]["fin"])) == (9, 0)
