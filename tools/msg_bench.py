#!/usr/bin/env python3
"""fws_gpu_decode_messages against its parts, warm, HIP events around
back-to-back calls, four rotating sources and destinations (the wire copies
total past the 256 MB Infinity Cache), on two workloads of the same byte volume:
  (a) c3     the BASELINE C3 mixed stream (one BIN frame per message);
  (b) frag   every message TEXT, split into 2 to 8 fragments, a PING every 64
             frames (payload sizes drawn as C3's: log-uniform 64 B .. 64 KiB).
Per workload, microseconds per call (median of the rounds):
  messages   fws_gpu_decode_messages
  stream     fws_gpu_decode_stream on the same bytes (in place, no UTF-8)
  parse      the parse alone (fws_internal_decode_parse)
  gather     fws_gpu_unmask_gather over the data frames' descriptors
  utf8       fws_gpu_validate_utf8 over the reassembled messages in dst
and messages / (parse + gather + utf8). One JSON line per workload.
usage: python tools/msg_bench.py [--target MiB] [--rounds R] [--steps K] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import struct
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flashws_amd import _lib, gpu  # noqa: E402


def header(opcode, fin, n, key):
    b0 = (fin << 7) | opcode
    if n < 126:
        h = bytes([b0, 0x80 | n])
    elif n <= 65535:
        h = bytes([b0, 0x80 | 126]) + struct.pack(">H", n)
    else:
        h = bytes([b0, 0x80 | 127]) + struct.pack(">Q", n)
    return h + struct.pack("<I", key)


def fragmented_stream(target, seed=42):
    """(wire, data-frame descriptors, message regions in dst) of workload (b)."""
    rng = np.random.default_rng(seed)
    frames = []                                       # (opcode, fin, length)
    msgs, total, nf = [], 0, 0
    while total < target:
        n = int(np.exp(rng.uniform(np.log(64), np.log(65536))))
        k = int(rng.integers(2, 9))
        cuts = np.sort(rng.integers(0, n + 1, k - 1)).tolist()
        for j, (a, b) in enumerate(zip([0] + cuts, cuts + [n])):
            if nf % 64 == 63:
                frames.append((9, 1, 8))
                nf += 1
            frames.append((1 if j == 0 else 0, int(j == k - 1), b - a))
            nf += 1
        msgs.append((total, n))
        total += n
    size = sum(6 + (0 if n < 126 else 2 if n <= 65535 else 8) + n for _, _, n in frames)
    wire = np.empty(size, dtype=np.uint8)
    text = rng.integers(0x20, 0x7F, total, dtype=np.uint8)      # ASCII: well-formed UTF-8
    descs = np.zeros(sum(1 for f in frames if f[0] < 8), dtype=_lib.FRAME_DESC)
    pos = src = d = 0
    for op, fin, n in frames:
        key = int(rng.integers(0, 1 << 32))
        h = header(op, fin, n, key)
        wire[pos:pos + len(h)] = np.frombuffer(h, dtype=np.uint8)
        pos += len(h)
        kb = np.resize(np.frombuffer(struct.pack("<I", key), dtype=np.uint8), n)
        if op < 8:
            wire[pos:pos + n] = text[src:src + n] ^ kb
            descs[d] = (pos, n, key, 0)
            src += n
            d += 1
        else:
            wire[pos:pos + n] = kb                   # a PING of zero bytes
        pos += n
    regions = np.zeros(len(msgs), dtype=_lib.FRAME_DESC)
    regions["payload_off"] = [m[0] for m in msgs]
    regions["payload_len"] = [m[1] for m in msgs]
    return wire, descs, regions, len(frames)


def c3_stream(target):
    wire, descs, _ = gpu.config_c3(target=target)
    regions = np.zeros(len(descs), dtype=_lib.FRAME_DESC)
    regions["payload_len"] = descs["payload_len"]
    regions["payload_off"] = np.concatenate(([0], np.cumsum(descs["payload_len"])[:-1]))
    return wire, descs, regions, len(descs)


def timed(fn, steps, warm=10):
    for i in range(warm):
        fn(i)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(steps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def bench(name, wire, descs, regions, n_frames, rounds, steps):
    L = _lib.lib()
    dev = torch.device("cuda:0")
    cap = n_frames + 64
    ctx = gpu.Ctx(0, max_frames=cap, max_stream_bytes=len(wire))
    srcs = [torch.from_numpy(wire).to(dev) for _ in range(4)]
    scratch = [torch.from_numpy(wire).to(dev) for _ in range(4)]           # decoded in place by `stream`
    total = int(descs["payload_len"].sum())
    dsts = [torch.empty(total + 64, dtype=torch.uint8, device=dev) for _ in range(4)]
    ctl = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    frames = torch.empty(cap * _lib.FRAME_INFO.itemsize, dtype=torch.uint8, device=dev)
    msgs = torch.empty(cap * _lib.MSG_INFO.itemsize, dtype=torch.uint8, device=dev)
    res = torch.empty(_lib.DECODE_RESULT.itemsize, dtype=torch.uint8, device=dev)
    mres = torch.empty(_lib.MSG_RESULT.itemsize, dtype=torch.uint8, device=dev)
    dd, rd = gpu.descs_to_device(descs, dev), gpu.descs_to_device(regions, dev)
    ok = torch.empty(len(regions) + 1, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream()
    parse = L.fws_internal_decode_parse
    parse.restype = C.c_int
    parse.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]

    def f_messages(i):
        rc, *_ = gpu.decode_messages(ctx, srcs[i % 4], cap, cap, dsts[i % 4], ctl, frames=frames, msgs=msgs,
                                     result=res, msg_result=mres)
        assert rc == 0

    def f_stream(i):
        rc, *_ = gpu.decode_stream(ctx, scratch[i % 4], cap, frames=frames, result=res)
        assert rc == 0

    def f_parse(i):
        assert parse(ctx.h, srcs[i % 4].data_ptr(), len(wire), frames.data_ptr(), cap, res.data_ptr(),
                     s.cuda_stream) == 0

    def f_gather(i):
        gpu.unmask_gather(ctx, dsts[i % 4], srcs[i % 4], dd, len(descs))

    def f_utf8(i):
        gpu.validate_utf8(ctx, dsts[i % 4], rd, len(regions), ok)

    # one checked call first: the result the timing is about
    f_messages(0)
    r = gpu.read_msg_result(mres)
    assert int(r["status"]) == 0 and int(r["n_msgs"]) >= len(regions) and int(r["data_bytes"]) == total, r
    m = gpu.read_messages(msgs, int(r["n_msgs"]))
    data = m[m["opcode"] < 8]
    assert np.array_equal(data["off"], regions["payload_off"]) and np.array_equal(data["len"], regions["payload_len"])
    for i in range(4):
        f_gather(i)                                   # every dst filled for the UTF-8 pass
    forms = {"messages": f_messages, "stream": f_stream, "parse": f_parse, "gather": f_gather, "utf8": f_utf8}
    times = {k: [] for k in forms}
    for rnd in range(rounds):
        for k in (list(forms) if rnd % 2 == 0 else list(forms)[::-1]):
            times[k].append(timed(forms[k], steps))
    out = {"workload": name, "wire_bytes": len(wire), "payload_bytes": total, "frames": n_frames,
           "messages": int(r["n_msgs"]), "rounds": rounds, "steps": steps,
           "device": torch.cuda.get_device_name(0)}
    for k in forms:
        out[k + "_us"] = round(statistics.median(times[k]), 2)
        out[k + "_us_min_max"] = [round(min(times[k]), 2), round(max(times[k]), 2)]
    parts = out["parse_us"] + out["gather_us"] + out["utf8_us"]
    out["messages_over_parts"] = round(out["messages_us"] / parts, 4)
    out["messages_over_stream"] = round(out["messages_us"] / out["stream_us"], 4)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--target", type=int, default=256, help="payload MiB per workload")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--only", default="", help="c3 or frag")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    target = a.target << 20
    lines = []
    for name, make in (("c3", c3_stream), ("frag", fragmented_stream)):
        if a.only and a.only != name:
            continue
        out = bench(name, *make(target), a.rounds, a.steps)
        print(json.dumps(out), flush=True)
        lines.append(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
