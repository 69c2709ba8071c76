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

--carry measures fws_gpu_decode_messages_carry instead:
  (i)  carry_cost   workload (b) whole in one call: the carry form and this
       tree's fws_gpu_decode_messages against the same call of a library built
       from the parent commit (--parent-lib), two contexts of which give the
       A/A spread; the forms alternate within every round.
  (ii) carry_reads  the stream cut into --read-mib reads at arbitrary byte
       offsets, decoded by the carry protocol (each call from the last
       resume_off: the unfinished frame) and by the resubmit protocol of the
       old call (from the open message's first header), each call's bytes
       first copied to a 16-B aligned buffer, as a caller must. Total device
       time per pass of the whole stream and the bytes each protocol parsed;
       for workload (b) and for one BIN message of the same size in 64 KiB
       fragments (BASELINE config 4's shape). The buffers of both protocols are
       worked out on the host from the frame list and checked against every
       call's resume_off in an untimed pass first.
--multi measures fws_gpu_decode_messages_multi: n connections
x one read each of 1 / 4 / 16 / 64 KiB (n in 1, 8, 64, 512, 4096), TEXT messages
fragmented as workload (b) with payloads up to half the read, every read made
of whole messages so the carries return to "closed" and every pass is the
same work. One multi call against the n sequential
fws_gpu_decode_messages_carry calls on the same reads and carries (that code is
the parent commit's: the baseline), alternating within each round, and a
device-to-device copy of the same bytes as a bandwidth reference; max_len is
the read size, so the small kernel form is the one measured on small reads.
Before timing, the two paths' outputs are compared byte for byte. Reads repeat
after 64 distinct ones. One JSON line per grid point.
--flow measures fws_gpu_decode_messages_flow:
  (i)  flow_cost    the --multi grid's whole-message reads (1 / 4 / 16 / 64 KiB x
       n = 1, 64, 512) through the flow call and this tree's multi call against
       the multi call of a library built from the parent commit (--parent-lib),
       two contexts of which give the A/A spread; the forms alternate within
       every round, and every form's outputs are compared byte for byte first.
       A parent library that has the flow call gives it a second A/A pair.
  (ii) flow_frames  n connections each receive one 1 MiB frame in 16 KiB reads:
       the flow protocol (every read uploaded once, one launch per step for all
       connections) against the only alternative today, the frame kept on the
       host and the carry call run on the growing buffer after every read.
       Total stream time per pass, uploads included, and bytes uploaded per
       connection; the flow parts joined are checked against the carry call's
       message first.
--tx-multi measures fws_gpu_encode_messages_multi: n
connections x one masked send each of 1 / 4 / 16 / 64 KiB in one frame (n in 1,
64, 512), and 64 x 64 KiB in frames of 4096 bytes. One multi call against what a
caller does today with the same library -- n fws_gpu_encode_frames calls, one
per connection into its own region, and one fws_gpu_encode_frames batch over
all frames (one back-to-back output the host must take apart) -- and a
device-to-device copy of the same bytes as a bandwidth reference; the forms
alternate within each round, and every form's output is compared byte for byte
first. max_len is the send size, so the small kernel form is the one measured
up to 16 KiB. One JSON line per grid point.
--reply measures fws_gpu_reply_messages_multi: n connections
(64, 512, 4096) x one read each holding one masked single-frame BIN message of
4 KiB (C1's shape; one send per connection, so the parent can express it), echoed.
  (i)  the loop, host wall time per step: flow decode -> synchronise -> the host
       builds fws_tx_send from the copied-back results and entries -> upload ->
       fws_gpu_encode_messages_multi -> synchronise, all calls from a library
       built from the parent commit (--parent-lib; two contexts give the A/A
       spread), against this tree's decode -> reply -> synchronise.
  (ii) the kernel alone, HIP events around back-to-back launches: the reply
       launch against the parent's fws_gpu_encode_messages_multi on unmasked
       one-frame sends of the same payloads (4 KiB and 64 KiB parts); the parent
       form runs twice per round for its own spread, and the reply launch once
       more with flags 0 (the entries, the scan and the table, no frame).
       A parent library that has the reply call is timed on it too, in both
       contexts, after its output was compared with this tree's.
The forms alternate within every round; both paths' output bytes are compared
first. One JSON line per grid point.
usage: python tools/msg_bench.py [--target MiB] [--rounds R] [--steps K] [--out FILE]
       python tools/msg_bench.py --carry [--parent-lib SO] [--read-mib M] [--target MiB] [--out FILE]
       python tools/msg_bench.py --multi [--grid-n N,N,..] [--grid-kib K,K,..] [--rounds R] [--out FILE]
       python tools/msg_bench.py --flow [--parent-lib SO] [--grid-n N,..] [--grid-kib K,..] [--rounds R] [--out FILE]
       python tools/msg_bench.py --tx-multi [--grid-n N,..] [--grid-kib K,..] [--rounds R] [--out FILE]
       python tools/msg_bench.py --reply --parent-lib SO [--grid-n N,..] [--grid-kib K,..] [--rounds R] [--out FILE]

--join measures fws_gpu_join_messages: n connections (64, 512,
4096) each receive one masked BIN message of two parts of 4 KiB (or 64 KiB) in
two reads, the cut inside the frame's payload.
  (i)  the loop, host wall time per step (both reads): flow decode -> copy back
       results, entries and dst -> synchronise -> the host keeps / joins the parts
       (two block copies: the least a host can do), all calls from a library built
       from the parent commit (--parent-lib; two contexts give the A/A spread),
       against this tree's decode -> join -> copy back results and records ->
       synchronise. The store is compared with the host's joined bytes first.
  (ii) the kernel alone, HIP events around back-to-back launches through raw
       pointers: the pair of join launches (the open part, then the part that
       completes the message), a device-to-device copy of the same bytes, and
       the empty call -- reads that hold one whole message, nothing to copy --
       against fws_gpu_reply_messages_multi with flags 0 on the same reads, the
       launch floor of a sibling, timed twice per round for its spread.
       python tools/msg_bench.py --join --parent-lib SO [--grid-n N,..] [--grid-kib K,..] [--rounds R] [--out FILE]

--publish measures fws_gpu_publish_messages: BIN messages in one
source buffer fanned out to every member of their room, one region per member.
  a  1 message of 4 KiB to 4,096 subscribers
  b  1 message of 64 KiB to 1,024 subscribers
  c  64 messages of 128 B to 4,096 subscribers (one list; seam-heavy)
  d  8 rooms of 512 members, 4 messages of 1 KiB per room
HIP events around back-to-back launches through raw pointers, at least 100 steps
after 10 of warm-up, rotating four output arenas; within each round, alternating:
the publish call; a device-to-device copy of one arena into the next (the same
bytes written); and, for a and b, fws_gpu_encode_messages_multi of a library
built from the parent commit (--parent-lib) on n one-frame server sends that
share one src_off, in two contexts (the A/A spread). Every region is compared
with the room's frames first, and with the parent's output. bytes_moved = the
distinct source bytes once + the region bytes, held against 8 TB/s.
       python tools/msg_bench.py --publish [--parent-lib SO] [--cases a,b,c,d] [--rounds R] [--steps S] [--out FILE]

--reply-strict measures fws_gpu_reply_messages_strict: the
echo of --reply (ii) with no failing item, n in {64, 512, 4096} x 4 KiB and 512
x 64 KiB, and one row where every read is a CLOSE of one byte and fails. HIP
events around back-to-back launches through raw pointers; within each round,
alternating: this tree's fws_gpu_reply_messages_multi, the same call of a
library built from the parent commit in two contexts (the A/A spread), and the
strict call -- and the parent's strict call in both contexts where it has one.
Every form's output is compared byte for byte first. SO is the parent commit's
library.
       python tools/msg_bench.py --reply-strict --parent-lib SO [--rounds R] [--steps S] [--out FILE]

--reply-client measures fws_gpu_reply_messages_multi_client / _strict_client
 on --reply's grid (n in {64, 512, 4096} x 4 KiB, {64, 512} x
64 KiB), one decoded single-frame BIN message per read, echoed. HIP events
around back-to-back launches through raw pointers; within each round,
alternating, all on the same decode output:
  k_reply, k_reply_strict                 this tree's server (unmasked) calls
  k_reply_parent_a/b, k_reply_strict_parent_a/b   the same calls of a library
                                          built from the parent commit, in two
                                          contexts: the A/A spread. This tree's
                                          server instantiations pass when within
                                          twice that spread of the parent.
  k_reply_client, k_reply_strict_client   the masked calls, same parts
  k_tx_multi_masked                       fws_gpu_encode_messages_multi on masked
                                          one-frame sends of the same payloads
Checked first, byte for byte: this tree's unmasked output against the
parent's, and the masked reply's region against the masked encode's (same keys).
--flow-client measures fws_gpu_decode_messages_flow_client on --flow (i)'s reads
with the masks and keys taken out (the same payloads, 4 bytes less per frame)
against fws_gpu_decode_messages_flow on the masked reads, this tree's and the
parent library's in two contexts (k_msg_flow's no-regression check). The
client's dst, ctl and entries are compared with the server's first.
       python tools/msg_bench.py --reply-client --parent-lib SO [--rounds R] [--steps S] [--out FILE]
       python tools/msg_bench.py --flow-client --parent-lib SO [--grid-n N,..] [--grid-kib K,..] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import struct
import sys
import time

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


def one_message_stream(target, frag=65536, seed=7):
    """One BIN message of `target` bytes in `frag`-byte fragments (BASELINE config 4's shape)."""
    rng = np.random.default_rng(seed)
    n = target // frag
    hdr = len(header(0, 0, frag, 0))
    wire = rng.integers(0, 256, n * (hdr + frag), dtype=np.uint8)
    for j in range(n):
        h = header(2 if j == 0 else 0, int(j == n - 1), frag, int(rng.integers(0, 1 << 32)))
        wire[j * (hdr + frag):j * (hdr + frag) + hdr] = np.frombuffer(h, dtype=np.uint8)
    return wire


def walk(wire):
    """The frame list of a well-formed stream: per frame (hdr_off, end, the first
    header of its message -- its own for a control frame --, whether a message is
    open after it and that message's first header)."""
    out, pos, n, msg0, is_open = [], 0, len(wire), 0, False
    while pos < n:
        b0, l7 = int(wire[pos]), int(wire[pos + 1]) & 127
        h, ln = 6, l7
        if l7 == 126:
            h, ln = 8, int.from_bytes(wire[pos + 2:pos + 4].tobytes(), "big")
        elif l7 == 127:
            h, ln = 14, int.from_bytes(wire[pos + 2:pos + 10].tobytes(), "big")
        op = b0 & 15
        if op in (1, 2):
            msg0 = pos
        if op < 8:
            is_open = not b0 >> 7
        out.append((pos, pos + h + ln, msg0 if op < 8 else pos, is_open, msg0))
        pos += h + ln
    return out


def read_buffers(wire, cuts):
    """Per protocol, the (start, end) of every call's bytes when the stream arrives cut at `cuts`."""
    fr = walk(wire)
    starts = np.array([f[0] for f in fr])
    carry, old, a, b = [], [], 0, 0
    for c in list(cuts) + [len(wire)]:
        carry.append((a, c))
        old.append((b, c))
        k = int(np.searchsorted(starts, c, side="right")) - 1    # the frame holding byte c - 0 (c > 0)
        hdr_off, end, m0, is_open, open0 = fr[k]
        if c >= end:                                  # on a frame boundary: nothing left of frame k
            a, b = c, (open0 if is_open else c)
        elif c - hdr_off < (6 if end - hdr_off < 132 else 8 if end - hdr_off < 65550 else 14):
            # inside frame k's header: the parse stops before it, the state is frame k - 1's
            a = hdr_off
            b = fr[k - 1][4] if k and fr[k - 1][3] else hdr_off
        else:                                         # inside its payload
            a = hdr_off
            open_before = k and fr[k - 1][3]
            b = m0 if (wire[hdr_off] & 15) < 8 else (fr[k - 1][4] if open_before else hdr_off)
    return carry, old


def carry_cost(wire, n_frames, parent_lib, rounds, steps):
    dev = torch.device("cuda:0")
    cap = n_frames + 64
    P = C.CDLL(parent_lib)
    for name, res, args in _lib.SIGNATURES:
        if hasattr(P, name):
            getattr(P, name).restype, getattr(P, name).argtypes = res, args
    assert not hasattr(P, "fws_gpu_decode_messages_carry"), "--parent-lib is this tree's library"
    srcs = [torch.from_numpy(wire).to(dev) for _ in range(4)]
    dsts = [torch.empty(len(wire), dtype=torch.uint8, device=dev) for _ in range(4)]
    ctl = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    u8 = dict(dtype=torch.uint8, device=dev)
    frames, msgs = torch.empty(cap * 24, **u8), torch.empty(cap * 32, **u8)
    res, mres, carry = torch.empty(40, **u8), torch.empty(64, **u8), torch.zeros(64, **u8)
    s = torch.cuda.current_stream()
    ctx = gpu.Ctx(0, max_frames=cap, max_stream_bytes=len(wire))
    pctx = []
    for _ in range(2):
        h = C.c_void_p()
        assert P.fws_gpu_ctx_create(0, C.byref(h)) == 0 and P.fws_gpu_ctx_reserve(h, cap, len(wire)) == 0
        pctx.append(h)

    def parent(h):
        def f(i):
            assert P.fws_gpu_decode_messages(h, srcs[i % 4].data_ptr(), len(wire), frames.data_ptr(), cap,
                                             msgs.data_ptr(), cap, dsts[i % 4].data_ptr(), len(wire), ctl.data_ptr(),
                                             1 << 20, res.data_ptr(), mres.data_ptr(), s.cuda_stream) == 0
        return f

    def f_new_old(i):
        assert gpu.decode_messages(ctx, srcs[i % 4], cap, cap, dsts[i % 4], ctl, frames=frames, msgs=msgs, result=res,
                                   msg_result=mres)[0] == 0

    def f_carry(i):
        assert gpu.decode_messages_carry(ctx, srcs[i % 4], cap, cap, dsts[i % 4], ctl, carry, frames=frames,
                                         msgs=msgs, result=res, msg_result=mres)[0] == 0

    forms = {"parent_a": parent(pctx[0]), "parent_b": parent(pctx[1]), "messages": f_new_old, "carry": f_carry}
    want = None
    for k, f in forms.items():                        # the same result from every form
        f(0)
        r = gpu.read_msg_result(mres)
        got = (int(r["status"]), int(r["n_msgs"]), int(r["data_bytes"]), dsts[0][:1 << 20].cpu().numpy().tobytes())
        want = want or got
        assert got == want and got[0] == 0, k
    times = {k: [] for k in forms}
    for rnd in range(rounds):
        for k in (list(forms) if rnd % 2 == 0 else list(forms)[::-1]):
            times[k].append(timed(forms[k], steps))
    out = {"measure": "carry_cost", "workload": "frag", "wire_bytes": len(wire), "frames": n_frames,
           "messages": want[1], "rounds": rounds, "steps": steps, "device": torch.cuda.get_device_name(0),
           "parent_lib": os.path.basename(parent_lib)}
    for k in forms:
        out[k + "_us"] = round(statistics.median(times[k]), 2)
        out[k + "_us_min_max"] = [round(min(times[k]), 2), round(max(times[k]), 2)]
    out["aa_spread_us"] = round(abs(out["parent_a_us"] - out["parent_b_us"]), 2)
    out["carry_minus_parent_us"] = round(out["carry_us"] - min(out["parent_a_us"], out["parent_b_us"]), 2)
    for h in pctx:
        P.fws_gpu_ctx_destroy(h)
    ctx.close()
    return out


def carry_reads(name, wire, read_bytes, rounds, seed=11):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(seed)
    n = len(wire)
    cuts = sorted(set(int(c) + int(rng.integers(-4096, 4096)) for c in range(read_bytes, n, read_bytes)))
    bufs = dict(zip(("carry", "resubmit"), read_buffers(wire, cuts)))
    fr = walk(wire)
    ends = np.array([f[1] for f in fr])
    starts = np.array([f[0] for f in fr])
    src = torch.from_numpy(wire).to(dev)
    u8 = dict(dtype=torch.uint8, device=dev)
    out = {"measure": "carry_reads", "workload": name, "wire_bytes": n, "frames": len(fr), "read_bytes": read_bytes,
           "calls": len(cuts) + 1, "rounds": rounds, "device": torch.cuda.get_device_name(0)}
    run = {}
    for proto, bl in bufs.items():
        longest = max(b - a for a, b in bl)
        cap = max(int(np.searchsorted(starts, b) - np.searchsorted(starts, a)) for a, b in bl) + 64
        ctx = gpu.Ctx(0, max_frames=cap, max_stream_bytes=longest)
        buf, dst = torch.empty(longest + 16, **u8), torch.empty(longest + 16, **u8)
        ctl = torch.empty(1 << 20, **u8)
        frames, msgs = torch.empty(cap * 24, **u8), torch.empty(cap * 32, **u8)
        res, mres, carry = torch.empty(40, **u8), torch.empty(64, **u8), torch.zeros(64, **u8)

        def one(a, b, proto=proto, ctx=ctx, buf=buf, dst=dst, ctl=ctl, frames=frames, msgs=msgs, res=res, mres=mres,
                carry=carry, cap=cap):
            buf[:b - a].copy_(src[a:b])               # the caller's move to an aligned buffer
            if proto == "carry":
                rc = gpu.decode_messages_carry(ctx, buf, cap, cap, dst, ctl, carry, frames=frames, msgs=msgs,
                                               result=res, msg_result=mres, n=b - a)[0]
            else:
                rc = gpu.decode_messages(ctx, buf, cap, cap, dst, ctl, frames=frames, msgs=msgs, result=res,
                                         msg_result=mres, n=b - a)[0]
            assert rc == 0

        # untimed, checked: every call resumes where the host walk says, every unit is delivered
        delivered = 0
        for j, (a, b) in enumerate(bl):
            one(a, b)
            r = gpu.read_msg_result(mres)
            nxt = bl[j + 1][0] if j + 1 < len(bl) else n
            assert int(r["status"]) == 0 and a + int(r["resume_off"]) == nxt, (proto, j, a, int(r["resume_off"]), nxt)
            delivered += int(r["n_msgs"])
        if proto == "carry":
            c = gpu.read_msg_carry(carry)
            assert int(c["wire_bytes"]) == n and int(c["n_msgs"]) == delivered and int(c["open_opcode"]) == 0
        out[proto + "_entries"] = delivered
        out[proto + "_bytes_parsed"] = int(sum(b - a for a, b in bl))
        out[proto + "_longest_call_bytes"] = int(longest)
        run[proto] = (one, bl, carry, ctx)
    times = {k: [] for k in run}
    for rnd in range(rounds + 1):                     # (round 0 warms up)
        for proto in (list(run) if rnd % 2 == 0 else list(run)[::-1]):
            one, bl, carry, _ = run[proto]
            carry.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for a, b in bl:
                one(a, b)
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                times[proto].append(e0.elapsed_time(e1) * 1e3)
    for proto in run:
        out[proto + "_total_us"] = round(statistics.median(times[proto]), 1)
        out[proto + "_total_us_min_max"] = [round(min(times[proto]), 1), round(max(times[proto]), 1)]
        run[proto][3].close()
    out["resubmit_over_carry"] = round(out["resubmit_total_us"] / out["carry_total_us"], 3)
    return out


def multi_read(rng, size):
    """One read of exactly `size` bytes (>= 1 KiB): whole TEXT messages in 2 to 8
    fragments, payloads log-uniform 64 B .. size / 2, a PING every 64 frames, at
    most 240 frames, the rest filled by one single-frame TEXT message. Returns (bytes, frames)."""
    parts, total, nf = [], 0, 0

    def put(op, fin, n, form126=False):
        nonlocal total, nf
        key = int(rng.integers(0, 1 << 32))
        h = header(op, fin, n, key)
        if form126 and n < 126:
            h = bytes([(fin << 7) | op, 0x80 | 126]) + struct.pack(">H", n) + struct.pack("<I", key)
        kb = np.resize(np.frombuffer(struct.pack("<I", key), dtype=np.uint8), n)
        body = rng.integers(0x20, 0x7F, n, dtype=np.uint8) ^ kb if op < 8 else kb
        parts.append(h + body.tobytes())
        total += len(h) + n
        nf += 1

    while True:
        n = int(np.exp(rng.uniform(np.log(64), np.log(size // 2))))
        k = int(rng.integers(2, 9))
        if total + n + 8 * k + 14 + 134 > size or nf + k + 2 > 240:
            break
        cuts = np.sort(rng.integers(0, n + 1, k - 1)).tolist()
        for j, (a, b) in enumerate(zip([0] + cuts, cuts + [n])):
            if nf % 64 == 63:
                put(9, 1, 8)
            put(1 if j == 0 else 0, int(j == k - 1), b - a)
    rem = size - total                                # >= 134: an 8-byte header
    put(1, 1, rem - 8, form126=True)
    wire = b"".join(parts)
    assert len(wire) == size
    return wire, nf


def multi_bench(n, size, rounds, steps):
    L = _lib.lib()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1000 * n + size)
    distinct = [multi_read(rng, size) for _ in range(min(n, 64))]
    cap = max(f for _, f in distinct) + 4
    assert cap <= _lib.FWS_MSG_MULTI_MAX_FRAMES
    ctl_cap = 8 * (cap // 64 + 2)
    host = np.stack([np.frombuffer(w, dtype=np.uint8) for w, _ in distinct])
    host = host[np.arange(n) % len(distinct)].reshape(-1)
    u8 = dict(dtype=torch.uint8, device=dev)
    wire = torch.from_numpy(host).to(dev)
    dst, dst2 = torch.zeros(n * size, **u8), torch.zeros(n * size, **u8)
    ctl = torch.zeros(n * ctl_cap, **u8)
    frames, msgs = torch.zeros(n * cap * 24, **u8), torch.zeros(n * cap * 32, **u8)
    res, mres, carries = torch.zeros(n * 40, **u8), torch.zeros(n * 64, **u8), torch.zeros(n * 64, **u8)
    desc = np.zeros(n, dtype=_lib.MSG_READ)
    for r in range(n):
        desc[r] = (r * size, r * size, r * ctl_cap, size, r, size, ctl_cap, r * cap, cap, r * cap, cap, 0)
    reads = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    ctx = gpu.Ctx(0, max_frames=cap, max_stream_bytes=size)
    s = torch.cuda.current_stream()
    seq = L.fws_gpu_decode_messages_carry
    p = {k: t.data_ptr() for k, t in dict(wire=wire, dst=dst, ctl=ctl, frames=frames, msgs=msgs, res=res, mres=mres,
                                          carries=carries).items()}

    def f_multi(i):
        assert gpu.decode_messages_multi(ctx, wire, reads, n, size, frames, msgs, dst, ctl, res, mres, carries, n) == 0

    def f_seq(i):
        h = s.cuda_stream
        for r in range(n):
            rc = seq(ctx.h, p["wire"] + r * size, size, p["frames"] + r * cap * 24, cap, p["msgs"] + r * cap * 32, cap,
                     p["dst"] + r * size, size, p["ctl"] + r * ctl_cap, ctl_cap, p["res"] + r * 40,
                     p["mres"] + r * 64, p["carries"] + r * 64, h)
            assert rc == 0

    def f_copy(i):
        dst2.copy_(wire)

    # checked first: both paths write the same bytes (n_survivors, a diagnostic, apart)
    snaps = []
    for f in (f_multi, f_seq):
        for t in (dst, ctl, frames, msgs, res, mres, carries):
            t.zero_()
        f(0)
        torch.cuda.synchronize()
        r = np.frombuffer(res.cpu().numpy().tobytes(), dtype=_lib.DECODE_RESULT).copy()
        r["n_survivors"] = 0
        snaps.append([t.clone() for t in (dst, ctl, frames, msgs, mres, carries)] + [r])
    m = np.frombuffer(snaps[0][4].cpu().numpy().tobytes(), dtype=_lib.MSG_RESULT)
    assert (m["status"] == 0).all() and (m["resume_off"] == size).all() and (m["open_opcode"] == 0).all()
    for a, b in zip(snaps[0][:-1], snaps[1][:-1]):
        assert torch.equal(a, b), "the multi call and the sequential calls differ"
    assert (snaps[0][-1] == snaps[1][-1]).all()
    forms = {"multi": (f_multi, steps), "seq": (f_seq, max(1, min(steps, 2048 // n))), "copy": (f_copy, steps)}
    times = {k: [] for k in forms}
    for rnd in range(rounds):
        for k in (list(forms) if rnd % 2 == 0 else list(forms)[::-1]):
            times[k].append(timed(forms[k][0], forms[k][1], warm=2 if k == "seq" else 10))
    out = {"measure": "multi", "n": n, "read_bytes": size, "form": "small" if size <= (16 << 10) else "full",
           "wire_bytes": n * size, "frames_per_read_max": cap - 4, "messages": int(m["n_msgs"].sum()),
           "rounds": rounds, "steps": {k: v[1] for k, v in forms.items()}, "device": torch.cuda.get_device_name(0)}
    for k in forms:
        out[k + "_us"] = round(statistics.median(times[k]), 2)
        out[k + "_us_min_max"] = [round(min(times[k]), 2), round(max(times[k]), 2)]
    out["seq_over_multi"] = round(out["seq_us"] / out["multi_us"], 2)
    out["multi_over_copy"] = round(out["multi_us"] / out["copy_us"], 2)
    out["multi_wire_gb_s"] = round(n * size / out["multi_us"] / 1e3, 2)
    ctx.close()
    return out


def flow_cost(n, size, parent_lib, rounds, steps):
    """--flow (i): multi_bench's whole-message reads through the flow call, this
    tree's multi call and the parent library's multi call (two contexts: A/A)."""
    dev = torch.device("cuda:0")
    P = C.CDLL(parent_lib)
    for name, res_t, args in _lib.SIGNATURES:
        if hasattr(P, name):
            getattr(P, name).restype, getattr(P, name).argtypes = res_t, args
    parent_has_flow = hasattr(P, "fws_gpu_decode_messages_flow")
    rng = np.random.default_rng(1000 * n + size)
    distinct = [multi_read(rng, size) for _ in range(min(n, 64))]
    cap = max(f for _, f in distinct) + 4
    ctl_cap = 8 * (cap // 64 + 2)
    host = np.stack([np.frombuffer(w, dtype=np.uint8) for w, _ in distinct])
    host = host[np.arange(n) % len(distinct)].reshape(-1)
    u8 = dict(dtype=torch.uint8, device=dev)
    wire = torch.from_numpy(host).to(dev)
    dst, ctl = torch.zeros(n * size, **u8), torch.zeros(n * ctl_cap, **u8)
    frames, msgs = torch.zeros(n * cap * 24, **u8), torch.zeros(n * cap * 32, **u8)
    res, mres = torch.zeros(n * 40, **u8), torch.zeros(n * 64, **u8)
    carries, flows = torch.zeros(n * 64, **u8), torch.zeros(n * _lib.MSG_FLOW.itemsize, **u8)
    desc = np.zeros(n, dtype=_lib.MSG_READ)
    for r in range(n):
        desc[r] = (r * size, r * size, r * ctl_cap, size, r, size, ctl_cap, r * cap, cap, r * cap, cap, 0)
    reads = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    ctx = gpu.Ctx(0)
    s = torch.cuda.current_stream()
    pctx = []
    for _ in range(2):
        h = C.c_void_p()
        assert P.fws_gpu_ctx_create(0, C.byref(h)) == 0
        pctx.append(h)

    def parent(h, fn=P.fws_gpu_decode_messages_multi, state=carries):
        def f(i):
            assert fn(h, wire.data_ptr(), reads.data_ptr(), n, size, frames.data_ptr(), msgs.data_ptr(), dst.data_ptr(),
                      ctl.data_ptr(), res.data_ptr(), mres.data_ptr(), state.data_ptr(), n, s.cuda_stream) == 0
        return f

    # (this tree's calls through raw pointers as the parent's: at n = 1 the Python wrapper's argument conversion
    # showed as 0.2 us on a kernel that was the parent's)
    forms = {"parent_a": parent(pctx[0]), "parent_b": parent(pctx[1]),
             "multi": parent(ctx.h, _lib.lib().fws_gpu_decode_messages_multi),
             "flow": parent(ctx.h, _lib.lib().fws_gpu_decode_messages_flow, flows)}
    if parent_has_flow:                               # the parent's flow call, its own A/A pair
        forms.update({"flow_parent_" + x: parent(h, P.fws_gpu_decode_messages_flow, flows) for x, h in zip("ab", pctx)})
    want = None
    for k, f in forms.items():                        # checked first: every form writes the same bytes
        for t in (dst, ctl, frames, msgs, res, mres, carries, flows):
            t.zero_()
        f(0)
        torch.cuda.synchronize()
        state = flows.view(n, -1)[:, :64].reshape(-1) if k.startswith("flow") else carries
        got = [t.clone() for t in (dst, ctl, frames, msgs, res, mres, state)]
        want = want or got
        assert all(torch.equal(a, b) for a, b in zip(got, want)), k
    m = np.frombuffer(mres.cpu().numpy().tobytes(), dtype=_lib.MSG_RESULT)
    assert (m["status"] == 0).all() and (m["resume_off"] == size).all() and (m["open_opcode"] == 0).all()
    times = {k: [] for k in forms}
    for rnd in range(rounds):
        for k in (list(forms) if rnd % 2 == 0 else list(forms)[::-1]):
            times[k].append(timed(forms[k], steps))
    out = {"measure": "flow_cost", "n": n, "read_bytes": size, "form": "small" if size <= (16 << 10) else "full",
           "wire_bytes": n * size, "rounds": rounds, "steps": steps, "device": torch.cuda.get_device_name(0),
           "parent_lib": os.path.basename(parent_lib)}
    for k in forms:
        out[k + "_us"] = round(statistics.median(times[k]), 2)
        out[k + "_us_min_max"] = [round(min(times[k]), 2), round(max(times[k]), 2)]
    base = min(out["parent_a_us"], out["parent_b_us"])
    out["aa_spread_us"] = round(abs(out["parent_a_us"] - out["parent_b_us"]), 2)
    out["flow_minus_parent_us"] = round(out["flow_us"] - base, 2)
    out["multi_minus_parent_us"] = round(out["multi_us"] - base, 2)
    if parent_has_flow:
        out["flow_aa_spread_us"] = round(abs(out["flow_parent_a_us"] - out["flow_parent_b_us"]), 2)
        out["flow_minus_flow_parent_us"] = round(out["flow_us"] - min(out["flow_parent_a_us"], out["flow_parent_b_us"]), 2)
    for h in pctx:
        P.fws_gpu_ctx_destroy(h)
    ctx.close()
    return out


def flow_frames(n, frame_bytes, read_bytes, rounds):
    """--flow (ii): n connections each receive one BIN frame of frame_bytes on
    the wire (header included) in reads of read_bytes. The flow protocol uploads
    every read once and makes one launch per step for all connections; the
    alternative today keeps the unfinished frame on the host and, per read and
    connection, uploads the buffer so far and runs the carry call on it
    (MessageStream's protocol). Pinned host memory, uploads on the timed stream."""
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(5)
    steps = frame_bytes // read_bytes
    assert steps * read_bytes == frame_bytes and read_bytes % 16 == 0 and read_bytes <= _lib.FWS_MSG_MULTI_MAX_READ
    body = frame_bytes - 14
    streams = []
    for c in range(n):
        key = int(rng.integers(0, 1 << 32))
        streams.append(np.concatenate([np.frombuffer(header(2, 1, body, key), dtype=np.uint8),
                                       rng.integers(0, 256, body, dtype=np.uint8)]))
    host = torch.from_numpy(np.stack(streams)).pin_memory()              # [n, frame_bytes]
    by_step = torch.from_numpy(np.stack(streams).reshape(n, steps, read_bytes).transpose(1, 0, 2).copy()).pin_memory()
    u8 = dict(dtype=torch.uint8, device=dev)
    cap = 8
    # flow: one slot per connection
    wire, dst, ctl = torch.zeros(n * read_bytes, **u8), torch.zeros(n * read_bytes, **u8), torch.zeros(n * 64, **u8)
    frames, msgs = torch.zeros(n * cap * 24, **u8), torch.zeros(n * cap * 32, **u8)
    res, mres = torch.zeros(n * 40, **u8), torch.zeros(n * 64, **u8)
    flows = torch.zeros(n * _lib.MSG_FLOW.itemsize, **u8)
    desc = np.zeros(n, dtype=_lib.MSG_READ)
    for r in range(n):
        desc[r] = (r * read_bytes, r * read_bytes, r * 64, read_bytes, r, read_bytes, 64, r * cap, cap, r * cap, cap, 0)
    reads = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    whole = torch.zeros(n * frame_bytes, **u8)        # the parts as a caller would keep them
    # carry: one growing buffer
    cwire, cdst, cctl = torch.zeros(frame_bytes, **u8), torch.zeros(frame_bytes, **u8), torch.zeros(64, **u8)
    cfr, cms = torch.zeros(cap * 24, **u8), torch.zeros(cap * 32, **u8)
    cres, cmres, carries = torch.zeros(40, **u8), torch.zeros(64, **u8), torch.zeros(n * 64, **u8)
    ctx = gpu.Ctx(0, max_frames=cap, max_stream_bytes=frame_bytes)

    def flow_pass(keep=False):
        flows.zero_()
        for k in range(steps):
            wire.copy_(by_step[k].reshape(-1), non_blocking=True)
            assert gpu.decode_messages_flow(ctx, wire, reads, n, read_bytes, frames, msgs, dst, ctl, res, mres, flows,
                                            n) == 0
            if keep:
                whole.view(n, steps, read_bytes)[:, k].copy_(dst.view(n, read_bytes))

    def carry_pass(keep=None):
        carries.zero_()
        for k in range(steps):
            for c in range(n):
                m = (k + 1) * read_bytes
                cwire[:m].copy_(host[c, :m], non_blocking=True)
                rc = gpu.decode_messages_carry(ctx, cwire, cap, cap, cdst, cctl, carries[c * 64:(c + 1) * 64],
                                               frames=cfr, msgs=cms, result=cres, msg_result=cmres, n=m)[0]
                assert rc == 0
                if keep is not None and c == keep and k == steps - 1:
                    torch.cuda.synchronize()
                    return cdst[:body].clone(), gpu.read_msg_result(cmres)

    # checked first: the flow parts joined are the carry call's message
    flow_pass(keep=True)
    torch.cuda.synchronize()
    m = np.frombuffer(mres.cpu().numpy().tobytes(), dtype=_lib.MSG_RESULT)
    assert (m["status"] == 0).all() and (m["n_msgs"] == 1).all() and (m["open_opcode"] == 0).all()
    for c in (0, n - 1):
        want, r = carry_pass(keep=c)
        assert int(r["status"]) == 0 and int(r["n_msgs"]) == 1 and int(r["data_bytes"]) == body
        # (the flow parts: 14 bytes fewer in the first read, every later read whole)
        got = torch.cat([whole.view(n, steps, read_bytes)[c, 0, :read_bytes - 14],
                         whole.view(n, steps, read_bytes)[c, 1:].reshape(-1)])
        assert torch.equal(got, want), c
    passes = {"flow": flow_pass, "carry_growing": carry_pass}
    times = {k: [] for k in passes}
    for rnd in range(rounds + 1):                     # (round 0 warms up)
        for k in (list(passes) if rnd % 2 == 0 else list(passes)[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            passes[k]()
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                times[k].append(e0.elapsed_time(e1) * 1e3)
    out = {"measure": "flow_frames", "n": n, "frame_bytes": frame_bytes, "read_bytes": read_bytes, "steps": steps,
           "rounds": rounds, "device": torch.cuda.get_device_name(0),
           "flow_calls": steps, "carry_calls": steps * n,
           "flow_uploaded_per_conn": frame_bytes,
           "carry_uploaded_per_conn": read_bytes * steps * (steps + 1) // 2}
    for k in passes:
        out[k + "_total_us"] = round(statistics.median(times[k]), 1)
        out[k + "_total_us_min_max"] = [round(min(times[k]), 1), round(max(times[k]), 1)]
    out["carry_over_flow"] = round(out["carry_growing_total_us"] / out["flow_total_us"], 2)
    ctx.close()
    return out


def tx_multi_bench(n, size, max_frame, rounds, steps):
    """--tx-multi: n connections each send `size` bytes, masked, in frames of
    max_frame bytes (0: one frame): one fws_gpu_encode_messages_multi call against
    n fws_gpu_encode_frames calls (one per connection, into the same regions) and
    one fws_gpu_encode_frames batch over all frames (one back-to-back output)."""
    L = _lib.lib()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(77 * n + size + max_frame)
    cuts = [(o, min(max_frame, size - o)) for o in range(0, size, max_frame)] if max_frame else [(0, size)]
    k = len(cuts)
    hdr = [6 + (0 if ln < 126 else 2 if ln <= 65535 else 8) for _, ln in cuts]
    need = size + sum(hdr)
    slot = (need + 15) & ~15
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    u8 = dict(dtype=torch.uint8, device=dev)
    src = torch.from_numpy(rng.integers(0, 256, n * size, dtype=np.uint8)).to(dev)
    out_multi, out_seq = torch.zeros(n * slot, **u8), torch.zeros(n * slot, **u8)
    out_batch, copy_dst = torch.zeros(n * need + 16, **u8), torch.zeros(n * slot, **u8)
    sends = np.zeros(n, dtype=_lib.TX_SEND)
    descs = np.zeros(n * k, dtype=_lib.TX_DESC)
    for r in range(n):
        s = sends[r]
        s["src_off"], s["out_off"], s["len"], s["out_cap"], s["conn"], s["max_frame"] = r * size, r * slot, size, slot, \
            r, max_frame
        s["key"], s["frame_type"], s["last"], s["masked"] = keys[r], 2, 1, 1
        for j, (o, ln) in enumerate(cuts):                # what a caller builds today: fws_tx_next per frame
            descs[r * k + j] = (r * size + o, ln, _lib.FWS_TX_FRAG_KEY(int(keys[r]), j), 2 if j == 0 else 0,
                                int(j == k - 1), 1, 0)
    d_sends = torch.from_numpy(sends.view(np.uint8).copy()).to(dev)
    d_descs = torch.from_numpy(descs.view(np.uint8).copy()).to(dev)
    res = torch.zeros(n * _lib.TX_RESULT.itemsize, **u8)
    conns = torch.zeros(n * _lib.TX_CONN.itemsize, **u8)
    lens = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    ctx = gpu.Ctx(0, max_frames=n * k + 64, max_stream_bytes=n * slot + 4096)
    s = torch.cuda.current_stream()
    enc = L.fws_gpu_encode_frames
    p = dict(src=src.data_ptr(), out=out_seq.data_ptr(), descs=d_descs.data_ptr(), lens=lens.data_ptr())

    def f_multi(i):
        assert gpu.encode_messages_multi(ctx, out_multi, src, d_sends, n, size, None, res, conns, n) == 0

    def forced(threads):                              # one kernel form whatever max_len says (tuning hook)
        def f(i):
            L.fws_internal_set_tx_multi_threads(threads)
            f_multi(i)
            L.fws_internal_set_tx_multi_threads(0)
        return f

    def f_seq(i):
        h = s.cuda_stream
        for r in range(n):
            assert enc(ctx.h, p["out"] + r * slot, slot, p["src"], p["descs"] + r * k * 24, k, p["lens"] + 8 * r, h) == 0

    def f_batch(i):
        assert enc(ctx.h, out_batch.data_ptr(), n * need + 16, p["src"], p["descs"], n * k, p["lens"] + 8 * n,
                   s.cuda_stream) == 0

    def f_copy(i):
        copy_dst.copy_(out_multi)

    # checked first: every form writes the same frames
    for f in (f_multi, f_seq, f_batch):
        f(0)
    torch.cuda.synchronize()
    r_ = np.frombuffer(res.cpu().numpy().tobytes(), dtype=_lib.TX_RESULT)
    assert (r_["status"] == 0).all() and (r_["out_len"] == need).all() and (r_["n_frames"] == k).all()
    ln_ = lens.cpu().numpy()
    assert (ln_[:n] == need).all() and ln_[n] == n * need
    a = out_multi.view(n, slot)[:, :need]
    assert torch.equal(a, out_seq.view(n, slot)[:, :need]), "the multi call and the per-connection calls differ"
    assert torch.equal(a.reshape(-1), out_batch[:n * need]), "the multi call and the batch differ"
    for threads in (256, 1024):                       # either form writes what the default one wrote
        out_multi.zero_()
        forced(threads)(0)
        assert torch.equal(out_multi.view(n, slot)[:, :need], out_seq.view(n, slot)[:, :need]), threads
    forms = {"multi": (f_multi, steps), "multi_256": (forced(256), steps), "multi_1024": (forced(1024), steps),
             "seq": (f_seq, max(1, min(steps, 2048 // n))), "batch": (f_batch, steps), "copy": (f_copy, steps)}
    times = {name: [] for name in forms}
    for rnd in range(rounds):
        for name in (list(forms) if rnd % 2 == 0 else list(forms)[::-1]):
            times[name].append(timed(forms[name][0], forms[name][1], warm=2 if name == "seq" else 10))
    out = {"measure": "tx_multi", "n": n, "send_bytes": size, "max_frame": max_frame, "frames_per_send": k,
           "form": "small" if size <= (16 << 10) else "full", "wire_bytes": n * need, "rounds": rounds,
           "steps": {name: v[1] for name, v in forms.items()}, "device": torch.cuda.get_device_name(0)}
    for name in forms:
        out[name + "_us"] = round(statistics.median(times[name]), 2)
        out[name + "_us_min_max"] = [round(min(times[name]), 2), round(max(times[name]), 2)]
    out["seq_over_multi"] = round(out["seq_us"] / out["multi_us"], 2)
    out["batch_over_multi"] = round(out["batch_us"] / out["multi_us"], 2)
    out["multi_over_copy"] = round(out["multi_us"] / out["copy_us"], 2)
    out["multi_wire_gb_s"] = round(n * need / out["multi_us"] / 1e3, 2)
    ctx.close()
    return out


def walled(fn, steps, warm=10):
    """Host wall time per step, microseconds; fn ends in its own synchronisation."""
    for i in range(warm):
        fn(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / steps


def reply_bench(n, size, parent_lib, rounds, steps, loop=True):
    """--reply: see the module docstring. size: the message's payload bytes."""
    dev = torch.device("cuda:0")
    P = C.CDLL(parent_lib)
    for name, res_t, args in _lib.SIGNATURES:
        if hasattr(P, name):
            getattr(P, name).restype, getattr(P, name).argtypes = res_t, args
    parent_has_reply = hasattr(P, "fws_gpu_reply_messages_multi")
    rng = np.random.default_rng(31 * n + size)
    hdr = [header(2, 1, size, int(rng.integers(0, 1 << 32))) for _ in range(min(n, 64))]
    rlen = len(hdr[0]) + size
    slot = (rlen + 15) & ~15
    need = size + (2 if size < 126 else 4 if size <= 65535 else 10)
    oslot = (need + 15) & ~15
    host = np.zeros((n, slot), dtype=np.uint8)
    body = rng.integers(0, 256, (min(n, 64), size), dtype=np.uint8)
    for r in range(n):
        host[r, :len(hdr[0])] = np.frombuffer(hdr[r % 64], dtype=np.uint8)
        host[r, len(hdr[0]):rlen] = body[r % 64]
    u8 = dict(dtype=torch.uint8, device=dev)
    pin = dict(dtype=torch.uint8, pin_memory=True)
    cap, ctl_cap = 2, 16
    wire = torch.from_numpy(host.reshape(-1)).to(dev)
    dst, ctl = torch.zeros(n * slot, **u8), torch.zeros(n * ctl_cap, **u8)
    frames, msgs = torch.zeros(n * cap * 24, **u8), torch.zeros(n * cap * 32, **u8)
    res, mres = torch.zeros(n * 40, **u8), torch.zeros(n * 64, **u8)
    flows = torch.zeros(n * _lib.MSG_FLOW.itemsize, **u8)
    desc = np.zeros(n, dtype=_lib.MSG_READ)
    regions = np.zeros(n, dtype=_lib.REPLY_REGION)
    for r in range(n):
        desc[r] = (r * slot, r * slot, r * ctl_cap, rlen, r, slot, ctl_cap, r * cap, cap, r * cap, cap, 0)
        regions[r] = (r * oslot, oslot, 0, 0, 0, 0)
    reads = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    d_regions = torch.from_numpy(regions.view(np.uint8).copy()).to(dev)
    out_new, out_old = torch.zeros(n * oslot, **u8), torch.zeros(n * oslot, **u8)
    tres = torch.zeros(n * _lib.TX_RESULT.itemsize, **u8)
    conns_new, conns_old = torch.zeros(n * _lib.TX_CONN.itemsize, **u8), torch.zeros(n * _lib.TX_CONN.itemsize, **u8)
    states = torch.zeros(n * _lib.REPLY_STATE.itemsize, **u8)
    d_sends = torch.zeros(n * _lib.TX_SEND.itemsize, **u8)
    h_mres, h_msgs, h_sends = torch.zeros(n * 64, **pin), torch.zeros(n * cap * 32, **pin), \
        torch.zeros(n * _lib.TX_SEND.itemsize, **pin)
    v_mres = h_mres.numpy().view(_lib.MSG_RESULT)
    v_msgs = h_msgs.numpy().view(_lib.MSG_INFO).reshape(n, cap)
    v_sends = h_sends.numpy().view(_lib.TX_SEND)
    dst_off, out_off = desc["dst_off"].copy(), regions["out_off"].copy()
    conn_ids = np.arange(n, dtype=np.uint32)
    ctx = gpu.Ctx(0)
    s = torch.cuda.current_stream()
    pctx = []
    for _ in range(2):
        h = C.c_void_p()
        assert P.fws_gpu_ctx_create(0, C.byref(h)) == 0
        pctx.append(h)
    max_len = rlen

    def p_decode(h):
        assert P.fws_gpu_decode_messages_flow(h, wire.data_ptr(), reads.data_ptr(), n, max_len, frames.data_ptr(),
                                              msgs.data_ptr(), dst.data_ptr(), ctl.data_ptr(), res.data_ptr(),
                                              mres.data_ptr(), flows.data_ptr(), n, s.cuda_stream) == 0

    def p_encode(h):
        assert P.fws_gpu_encode_messages_multi(h, out_old.data_ptr(), dst.data_ptr(), d_sends.data_ptr(), n, size,
                                               None, tres.data_ptr(), conns_old.data_ptr(), n, s.cuda_stream) == 0

    def build_sends():
        """The host walk: one completed message per read, echoed as one send (vectorised over the reads)."""
        assert (v_mres["status"] == 0).all() and (v_mres["n_msgs"] == 1).all()
        e = v_msgs[:, 0]
        v_sends["src_off"], v_sends["out_off"], v_sends["len"] = dst_off + e["off"], out_off, e["len"]
        v_sends["out_cap"], v_sends["conn"], v_sends["max_frame"], v_sends["key"] = oslot, conn_ids, 0, 0
        v_sends["frame_type"], v_sends["last"], v_sends["masked"] = e["opcode"], 1, 0

    def old_loop(h):
        def f(i):
            p_decode(h)
            h_mres.copy_(mres, non_blocking=True)
            h_msgs.copy_(msgs, non_blocking=True)
            s.synchronize()
            build_sends()
            d_sends.copy_(h_sends, non_blocking=True)
            p_encode(h)
            s.synchronize()
        return f

    # (raw pointers, as the parent's calls above: the Python wrapper's argument conversion costs more host time
    # than a small launch takes on the device, and the events would time the host)
    reply_fn = _lib.lib().fws_gpu_reply_messages_multi
    rp = [t.data_ptr() for t in (reads, msgs, dst, ctl, mres, d_regions, out_new, tres, conns_new, states)]

    def f_reply(i, flags=_lib.FWS_REPLY_CONTROL | _lib.FWS_REPLY_ECHO, fn=reply_fn, h=None, out=rp[6], conns=rp[8]):
        assert fn(h or ctx.h, rp[0], n, max_len, rp[1], rp[2], rp[3], rp[4], rp[5], out, None, rp[7], conns,
                  rp[9], n, flags, s.cuda_stream) == 0

    decode_fn = _lib.lib().fws_gpu_decode_messages_flow
    dp = [t.data_ptr() for t in (wire, reads, frames, msgs, dst, ctl, res, mres, flows)]

    def new_loop(i):
        assert decode_fn(ctx.h, dp[0], dp[1], n, max_len, dp[2], dp[3], dp[4], dp[5], dp[6], dp[7], dp[8], n,
                         s.cuda_stream) == 0
        f_reply(i)
        s.synchronize()

    # checked first: both paths write the same frames
    old_loop(pctx[0])(0)
    new_loop(0)
    t = np.frombuffer(tres.cpu().numpy().tobytes(), dtype=_lib.TX_RESULT)
    assert (t["status"] == 0).all() and (t["out_len"] == need).all() and (t["n_frames"] == 1).all()
    assert torch.equal(out_new, out_old) and int(out_new.view(n, oslot)[:, 0].min()) == 0x82
    assert torch.equal(conns_new, conns_old)
    if parent_has_reply:                              # and the parent's reply call, into the old path's buffers
        for h in pctx:
            out_old.zero_(), conns_old.zero_()
            f_reply(0, fn=P.fws_gpu_reply_messages_multi, h=h, out=out_old.data_ptr(), conns=conns_old.data_ptr())
            assert torch.equal(out_new, out_old) and torch.equal(conns_new, conns_old)
    out = {"measure": "reply", "n": n, "part_bytes": size, "form": "small" if rlen <= (16 << 10) else "full",
           "reply_bytes": n * need, "rounds": rounds, "steps": steps, "device": torch.cuda.get_device_name(0),
           "parent_lib": os.path.basename(parent_lib)}
    forms = {}
    if loop:
        forms.update({"loop_parent_a": (walled, old_loop(pctx[0])), "loop_parent_b": (walled, old_loop(pctx[1])),
                      "loop_reply": (walled, new_loop)})
    forms.update({"k_tx_multi_a": (timed, lambda i: p_encode(pctx[0])), "k_tx_multi_b": (timed, lambda i: p_encode(pctx[1])),
                  "k_reply": (timed, f_reply),
                  # flags 0: the entries read, the scan and the table, no frame (where the time of a small call goes)
                  "k_reply_no_frames": (timed, lambda i: f_reply(i, 0))})
    if parent_has_reply:                              # the timed launches of all three write into one set of buffers
        forms.update({"k_reply_parent_" + x: (timed, lambda i, h=h: f_reply(i, fn=P.fws_gpu_reply_messages_multi, h=h))
                      for x, h in zip("ab", pctx)})
    times = {k: [] for k in forms}
    for rnd in range(rounds):
        for k in (list(forms) if rnd % 2 == 0 else list(forms)[::-1]):
            times[k].append(forms[k][0](forms[k][1], steps))
    for k in forms:
        out[k + "_us"] = round(statistics.median(times[k]), 2)
        out[k + "_us_min_max"] = [round(min(times[k]), 2), round(max(times[k]), 2)]
    if loop:
        base = min(out["loop_parent_a_us"], out["loop_parent_b_us"])
        out["loop_aa_spread_us"] = round(abs(out["loop_parent_a_us"] - out["loop_parent_b_us"]), 2)
        out["loop_parent_over_reply"] = round(base / out["loop_reply_us"], 2)
    kb = min(out["k_tx_multi_a_us"], out["k_tx_multi_b_us"])
    out["k_aa_spread_us"] = round(abs(out["k_tx_multi_a_us"] - out["k_tx_multi_b_us"]), 2)
    out["k_reply_over_tx_multi"] = round(out["k_reply_us"] / kb, 3)
    out["k_reply_gb_s"] = round(n * need / out["k_reply_us"] / 1e3, 2)
    if parent_has_reply:
        out["k_reply_aa_spread_us"] = round(abs(out["k_reply_parent_a_us"] - out["k_reply_parent_b_us"]), 2)
        out["k_reply_minus_parent_us"] = round(out["k_reply_us"] - min(out["k_reply_parent_a_us"],
                                                                        out["k_reply_parent_b_us"]), 2)
    for h in pctx:
        P.fws_gpu_ctx_destroy(h)
    ctx.close()
    return out


def join_bench(n, part, parent_lib, rounds, steps, loop=True):
    """--join: see the module docstring. part: the bytes of each of a message's two parts."""
    dev = torch.device("cuda:0")
    P = C.CDLL(parent_lib)
    for name, res_t, args in _lib.SIGNATURES:
        if hasattr(P, name):
            getattr(P, name).restype, getattr(P, name).argtypes = res_t, args
    assert not hasattr(P, "fws_gpu_join_messages"), "--parent-lib is this tree's library"
    L = _lib.lib()
    rng = np.random.default_rng(37 * n + part)
    size = 2 * part
    hl = len(header(2, 1, size, 0))
    body = rng.integers(0, 256, (min(n, 64), size), dtype=np.uint8)
    keys = [int(rng.integers(0, 1 << 32)) for _ in range(min(n, 64))]
    # read A: the header and the first part; read B: the second part; read W: a whole message of one part's size
    hw = len(header(2, 1, part, 0))
    lens = {"A": hl + part, "B": part, "W": hw + part}
    slot = (hl + part + 15) & ~15
    u8 = dict(dtype=torch.uint8, device=dev)
    pin = dict(dtype=torch.uint8, pin_memory=True)
    cap, ctl_cap = 2, 16
    sets = {}
    for name, ln in lens.items():
        host = np.zeros((n, slot), dtype=np.uint8)
        for r in range(n):
            kb = np.resize(np.frombuffer(struct.pack("<I", keys[r % 64]), dtype=np.uint8), size)
            msg = np.concatenate([np.frombuffer(header(2, 1, size, keys[r % 64]), dtype=np.uint8), body[r % 64] ^ kb])
            if name == "W":
                msg = np.concatenate([np.frombuffer(header(2, 1, part, keys[r % 64]), dtype=np.uint8),
                                      (body[r % 64] ^ kb)[:part]])
            host[r, :ln] = msg[hl + part:] if name == "B" else msg[:ln]
        desc = np.zeros(n, dtype=_lib.MSG_READ)
        for r in range(n):
            desc[r] = (r * slot, r * slot, r * ctl_cap, ln, r, slot, ctl_cap, r * cap, cap, r * cap, cap, 0)
        sets[name] = dict(len=ln, wire=torch.from_numpy(host.reshape(-1)).to(dev),
                          reads=torch.from_numpy(desc.view(np.uint8).copy()).to(dev), dst=torch.zeros(n * slot, **u8),
                          ctl=torch.zeros(n * ctl_cap, **u8), frames=torch.zeros(n * cap * 24, **u8),
                          msgs=torch.zeros(n * cap * 32, **u8), res=torch.zeros(n * 40, **u8),
                          mres=torch.zeros(n * 64, **u8), joined=torch.zeros(n * cap * 32, **u8),
                          jres=torch.zeros(n * 32, **u8))
    flows = {k: torch.zeros(n * _lib.MSG_FLOW.itemsize, **u8) for k in ("new", "old", "whole")}
    H = (size + 15) & ~15
    store = torch.zeros(n * 2 * H, **u8)
    jstates = {k: torch.zeros(n * 32, **u8) for k in ("new", "whole")}
    ctx = gpu.Ctx(0)
    s = torch.cuda.current_stream()
    pctx = []
    for _ in range(2):
        h = C.c_void_p()
        assert P.fws_gpu_ctx_create(0, C.byref(h)) == 0
        pctx.append(h)

    def decode(fn, h, name, fl):
        t = sets[name]
        assert fn(h, t["wire"].data_ptr(), t["reads"].data_ptr(), n, t["len"], t["frames"].data_ptr(),
                  t["msgs"].data_ptr(), t["dst"].data_ptr(), t["ctl"].data_ptr(), t["res"].data_ptr(),
                  t["mres"].data_ptr(), flows[fl].data_ptr(), n, s.cuda_stream) == 0

    def join(name, st):
        t = sets[name]
        assert L.fws_gpu_join_messages(ctx.h, t["reads"].data_ptr(), n, t["len"], t["msgs"].data_ptr(),
                                       t["dst"].data_ptr(), t["mres"].data_ptr(), store.data_ptr(), 2 * H,
                                       t["joined"].data_ptr(), t["jres"].data_ptr(), jstates[st].data_ptr(), n,
                                       s.cuda_stream) == 0

    # the parent's loop: every read's results, entries and dst come back and the host keeps the parts
    h_mres, h_msgs, h_dst = torch.zeros(n * 64, **pin), torch.zeros(n * cap * 32, **pin), torch.zeros(n * slot, **pin)
    v_mres, v_dst = h_mres.numpy().view(_lib.MSG_RESULT), h_dst.numpy().reshape(n, slot)
    v_msgs = h_msgs.numpy().view(_lib.MSG_INFO).reshape(n, cap)
    kept = np.zeros((n, part), dtype=np.uint8)
    host_joined = np.zeros((n, size), dtype=np.uint8)

    def old_loop(h):
        def f(i):
            for name in "AB":
                decode(P.fws_gpu_decode_messages_flow, h, name, "old")
                t = sets[name]
                h_mres.copy_(t["mres"], non_blocking=True)
                h_msgs.copy_(t["msgs"], non_blocking=True)
                h_dst.copy_(t["dst"], non_blocking=True)
                s.synchronize()
                assert (v_mres["status"] == 0).all()
                if name == "A":                          # the open part of every read (vectorised: same offsets)
                    assert (v_mres["open_len"] == part).all() and (v_mres["open_off"] == 0).all()
                    kept[:] = v_dst[:, :part]
                else:                                    # the CONTINUED entry completes it
                    assert (v_msgs[:, 0]["flags"] == 1).all() and (v_msgs[:, 0]["len"] == part).all()
                    host_joined[:, :part] = kept
                    host_joined[:, part:] = v_dst[:, :part]
        return f

    h_jres, h_joined = torch.zeros(n * 32, **pin), torch.zeros(n * cap * 32, **pin)
    v_jres = h_jres.numpy().view(_lib.JOIN_RESULT)

    def new_loop(i):
        for name in "AB":
            decode(L.fws_gpu_decode_messages_flow, ctx.h, name, "new")
            join(name, "new")
            h_jres.copy_(sets[name]["jres"], non_blocking=True)
            h_joined.copy_(sets[name]["joined"], non_blocking=True)
            s.synchronize()
            assert (v_jres["status"] == 0).all()

    # checked first: the store holds what the host joins
    old_loop(pctx[0])(0)
    new_loop(0)
    rec = h_joined.numpy().view(_lib.JOIN_INFO).reshape(n, cap)[:, 0]
    assert (rec["where"] == _lib.FWS_JOIN_IN_STORE).all() and (rec["len"] == size).all()
    assert (rec["off"] == np.arange(n, dtype=np.uint64) * np.uint64(2 * H)).all()
    got = store.cpu().numpy().reshape(n, 2 * H)[:, :size]
    assert np.array_equal(got, host_joined) and np.array_equal(got[:len(body)], body)
    # the whole-message reads for the empty call: decoded once, every record IN_DST, nothing copied
    decode(L.fws_gpu_decode_messages_flow, ctx.h, "W", "whole")
    join("W", "whole")
    s.synchronize()
    w = sets["W"]
    jr = np.frombuffer(w["jres"].cpu().numpy().tobytes(), dtype=_lib.JOIN_RESULT)
    assert (jr["status"] == 0).all() and (jr["n_joined"] == 1).all() and (jr["copied"] == 0).all()
    tres, conns = torch.zeros(n * _lib.TX_RESULT.itemsize, **u8), torch.zeros(n * _lib.TX_CONN.itemsize, **u8)
    rstates, regions = torch.zeros(n * _lib.REPLY_STATE.itemsize, **u8), np.zeros(n, dtype=_lib.REPLY_REGION)
    regions["out_off"], regions["out_cap"] = np.arange(n, dtype=np.uint64) * np.uint64(slot + 16), slot + 16
    d_regions, out = torch.from_numpy(regions.view(np.uint8).copy()).to(dev), torch.zeros(n * (slot + 16), **u8)

    def f_reply0(i):
        assert L.fws_gpu_reply_messages_multi(ctx.h, w["reads"].data_ptr(), n, w["len"], w["msgs"].data_ptr(),
                                              w["dst"].data_ptr(), w["ctl"].data_ptr(), w["mres"].data_ptr(),
                                              d_regions.data_ptr(), out.data_ptr(), None, tres.data_ptr(),
                                              conns.data_ptr(), rstates.data_ptr(), n, 0, s.cuda_stream) == 0

    def f_copy(i):                                       # the same bytes device to device: a bandwidth reference
        for name in "AB":
            store.view(n, 2 * H)[:, :part].copy_(sets[name]["dst"].view(n, slot)[:, :part])

    def f_join_ab(i):                                    # two launches: an open part, then the part that completes
        join("A", "new")
        join("B", "new")

    out_line = {"measure": "join", "n": n, "part_bytes": part, "form": "small" if lens["A"] <= (16 << 10) else "full",
                "copied_bytes_per_launch": n * part, "rounds": rounds, "steps": steps,
                "device": torch.cuda.get_device_name(0), "parent_lib": os.path.basename(parent_lib)}
    forms = {}
    if loop:
        forms.update({"loop_parent_a": (walled, old_loop(pctx[0])), "loop_parent_b": (walled, old_loop(pctx[1])),
                      "loop_join": (walled, new_loop)})
    forms.update({"k_join_pair": (timed, f_join_ab), "k_join_empty": (timed, lambda i: join("W", "whole")),
                  "k_reply_no_frames_a": (timed, f_reply0), "k_reply_no_frames_b": (timed, f_reply0),
                  "copy_pair": (timed, f_copy)})
    times = {k: [] for k in forms}
    for rnd in range(rounds):
        for k in (list(forms) if rnd % 2 == 0 else list(forms)[::-1]):
            times[k].append(forms[k][0](forms[k][1], steps))
    for k in forms:
        out_line[k + "_us"] = round(statistics.median(times[k]), 2)
        out_line[k + "_us_min_max"] = [round(min(times[k]), 2), round(max(times[k]), 2)]
    if loop:                                             # a step is both reads of the message
        base = min(out_line["loop_parent_a_us"], out_line["loop_parent_b_us"])
        out_line["loop_aa_spread_us"] = round(abs(out_line["loop_parent_a_us"] - out_line["loop_parent_b_us"]), 2)
        out_line["loop_parent_over_join"] = round(base / out_line["loop_join_us"], 2)
    out_line["k_join_us_per_launch"] = round(out_line["k_join_pair_us"] / 2, 2)
    out_line["k_join_gb_s"] = round(2 * n * part / out_line["k_join_pair_us"] / 1e3, 2)     # bytes copied (read + written once)
    out_line["copy_gb_s"] = round(2 * n * part / out_line["copy_pair_us"] / 1e3, 2)
    out_line["k_sibling_spread_us"] = round(abs(out_line["k_reply_no_frames_a_us"] - out_line["k_reply_no_frames_b_us"]), 2)
    out_line["k_join_empty_minus_sibling_us"] = round(
        out_line["k_join_empty_us"] - min(out_line["k_reply_no_frames_a_us"], out_line["k_reply_no_frames_b_us"]), 2)
    for h in pctx:
        P.fws_gpu_ctx_destroy(h)
    ctx.close()
    return out_line


PUBLISH_CASES = {"a": dict(rooms=1, members=4096, msgs=1, size=4 << 10), "b": dict(rooms=1, members=1024, msgs=1, size=64 << 10),
                 "c": dict(rooms=1, members=4096, msgs=64, size=128), "d": dict(rooms=8, members=512, msgs=4, size=1 << 10)}
PUBLISH_ARENAS = 4


def publish_bench(case, parent_lib, rounds, steps):
    """--publish: see the module docstring."""
    dev = torch.device("cuda:0")
    L = _lib.lib()
    p = PUBLISH_CASES[case]
    rooms, members, msgs, size = p["rooms"], p["members"], p["msgs"], p["size"]
    n, n_msgs = rooms * members, rooms * msgs
    rng = np.random.default_rng(ord(case))
    frame = size + 2 + (0 if size < 126 else 2 if size <= 65535 else 8)
    need = msgs * frame
    slot = (need + 15) & ~15
    u8 = dict(dtype=torch.uint8, device=dev)
    src_h = rng.integers(0, 256, n_msgs * size, dtype=np.uint8)
    src = torch.from_numpy(src_h).to(dev)
    recs = np.zeros(n_msgs, dtype=_lib.JOIN_INFO)
    for i in range(n_msgs):
        recs[i]["off"], recs[i]["len"], recs[i]["opcode"], recs[i]["where"] = i * size, size, 2, _lib.FWS_JOIN_IN_DST
    lst = np.arange(n_msgs, dtype=np.uint32)          # room r's list: its msgs records
    subs = np.zeros(n, dtype=_lib.PUB_SUB)
    for s in range(n):
        subs[s] = (s * slot, slot, s, (s // members) * msgs, msgs, 0, 0)
    d_recs, d_lst, d_subs = (torch.from_numpy(x.view(np.uint8).copy()).to(dev) for x in (recs, lst, subs))
    outs = [torch.zeros(n * slot, **u8) for _ in range(PUBLISH_ARENAS)]
    res, conns = torch.zeros(n * _lib.TX_RESULT.itemsize, **u8), torch.zeros(n * _lib.TX_CONN.itemsize, **u8)
    states = torch.zeros(n * _lib.REPLY_STATE.itemsize, **u8)
    ctx = gpu.Ctx(0, max_frames=64, max_stream_bytes=4096)
    h = torch.cuda.current_stream().cuda_stream
    ptr = dict(recs=d_recs.data_ptr(), lst=d_lst.data_ptr(), subs=d_subs.data_ptr(), src=src.data_ptr(),
               res=res.data_ptr(), conns=conns.data_ptr(), states=states.data_ptr(), outs=[o.data_ptr() for o in outs])
    pub = L.fws_gpu_publish_messages

    def f_publish(i):
        assert pub(ctx.h, ptr["recs"], n_msgs, ptr["src"], None, None, ptr["lst"], n_msgs, ptr["subs"], n, size,
                   ptr["outs"][i % PUBLISH_ARENAS], None, ptr["res"], ptr["conns"], ptr["states"], n, h) == 0

    def f_copy(i):                                    # the same bytes moved by a device-to-device copy
        outs[(i + 1) % PUBLISH_ARENAS].copy_(outs[i % PUBLISH_ARENAS])

    # checked first: every region holds the room's frames
    for i in range(PUBLISH_ARENAS):
        f_publish(i)
    torch.cuda.synchronize()
    r_ = np.frombuffer(res.cpu().numpy().tobytes(), dtype=_lib.TX_RESULT)
    assert (r_["status"] == 0).all() and (r_["out_len"] == need).all() and (r_["n_frames"] == msgs).all()
    hdr = header(2, 1, size, 0)[:-4]                  # a server frame's: no key, no MASK bit
    hdr = hdr[:1] + bytes([hdr[1] & 0x7F]) + hdr[2:]
    for r in range(rooms):
        want = b"".join(hdr + src_h[(r * msgs + j) * size:(r * msgs + j + 1) * size].tobytes() for j in range(msgs))
        want = torch.from_numpy(np.frombuffer(want, dtype=np.uint8).copy()).to(dev)
        for o in outs:
            got = o.view(n, slot)[r * members:(r + 1) * members, :need]
            assert torch.equal(got, want.expand(members, need)), "a region differs from the room's frames"
    forms = {"publish": f_publish, "copy": f_copy}
    parents = []
    if msgs == 1 and rooms == 1 and parent_lib:
        # the parent's way to the same bytes: n one-frame server sends that share one src_off
        P = C.CDLL(parent_lib)
        for name, res_t, args in _lib.SIGNATURES:
            if hasattr(P, name):
                getattr(P, name).restype, getattr(P, name).argtypes = res_t, args
        assert not hasattr(P, "fws_gpu_publish_messages"), "--parent-lib is this tree's library"
        sends = np.zeros(n, dtype=_lib.TX_SEND)
        for s in range(n):
            sends[s]["out_off"], sends[s]["len"], sends[s]["out_cap"], sends[s]["conn"] = s * slot, size, slot, s
            sends[s]["frame_type"], sends[s]["last"] = 2, 1
        d_sends = torch.from_numpy(sends.view(np.uint8).copy()).to(dev)
        out_p = [torch.zeros(n * slot, **u8) for _ in range(PUBLISH_ARENAS)]
        conns_p = torch.zeros(n * _lib.TX_CONN.itemsize, **u8)
        for tag in ("a", "b"):
            pc = C.c_void_p()
            assert P.fws_gpu_ctx_create(0, C.byref(pc)) == 0
            parents.append(pc)

            def f_parent(i, pc=pc):
                assert P.fws_gpu_encode_messages_multi(pc, out_p[i % PUBLISH_ARENAS].data_ptr(), ptr["src"],
                                                       d_sends.data_ptr(), n, size, None, ptr["res"],
                                                       conns_p.data_ptr(), n, h) == 0
            forms["encode_parent_" + tag] = f_parent
        for i in range(PUBLISH_ARENAS):
            forms["encode_parent_a"](i)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(outs, out_p)), "the publish and the parent's encode differ"
    times = {name: [] for name in forms}
    for rnd in range(rounds):
        for name in (list(forms) if rnd % 2 == 0 else list(forms)[::-1]):
            times[name].append(timed(forms[name], steps))
    moved = n_msgs * size + n * need                  # distinct source bytes once + region bytes
    out = {"measure": "publish", "case": case, "subscribers": n, "rooms": rooms, "msgs_per_list": msgs,
           "msg_bytes": size, "region_bytes": need, "form": "small" if size <= (16 << 10) else "full",
           "bytes_moved": moved, "rounds": rounds, "steps": steps, "arenas": PUBLISH_ARENAS,
           "device": torch.cuda.get_device_name(0), "parent_lib": os.path.basename(parent_lib) if parents else ""}
    for name in forms:
        out[name + "_us"] = round(statistics.median(times[name]), 2)
        out[name + "_us_min_max"] = [round(min(times[name]), 2), round(max(times[name]), 2)]
    out["publish_tb_s"] = round(moved / out["publish_us"] / 1e6, 3)
    out["publish_of_8tb_s_roofline"] = round(moved / out["publish_us"] / 1e6 / 8.0, 3)
    out["publish_over_copy"] = round(out["publish_us"] / out["copy_us"], 2)
    if parents:
        pa, pb = out["encode_parent_a_us"], out["encode_parent_b_us"]
        out["parent_spread_us"] = round(abs(pa - pb), 2)
        out["publish_minus_parent_us"] = round(out["publish_us"] - min(pa, pb), 2)
        out["publish_over_parent"] = round(out["publish_us"] / min(pa, pb), 3)
        for pc in parents:
            P.fws_gpu_ctx_destroy(pc)
    ctx.close()
    return out


def reply_strict_bench(n, size, parent_lib, rounds, steps, fail=False):
    """--reply-strict: see the module docstring. size: the message's payload
    bytes; fail: every read is a CLOSE frame of one byte instead, which the
    strict call answers with 1002 from its constant source."""
    dev = torch.device("cuda:0")
    P = C.CDLL(parent_lib)
    for name, res_t, args in _lib.SIGNATURES:
        if hasattr(P, name):
            getattr(P, name).restype, getattr(P, name).argtypes = res_t, args
    assert hasattr(P, "fws_gpu_reply_messages_multi"), "--parent-lib has no plain reply call"
    parent_has_strict = hasattr(P, "fws_gpu_reply_messages_strict")
    if fail:
        size = 1
    rng = np.random.default_rng(37 * n + size)
    hdr = [header(8 if fail else 2, 1, size, int(rng.integers(0, 1 << 32))) for _ in range(min(n, 64))]
    rlen = len(hdr[0]) + size
    slot = (rlen + 15) & ~15
    need = 4 if fail else size + (2 if size < 126 else 4 if size <= 65535 else 10)
    oslot = (max(need, size + 2) + 15) & ~15
    host = np.zeros((n, slot), dtype=np.uint8)
    body = rng.integers(0, 256, (min(n, 64), size), dtype=np.uint8)
    for r in range(n):
        host[r, :len(hdr[0])] = np.frombuffer(hdr[r % 64], dtype=np.uint8)
        host[r, len(hdr[0]):rlen] = body[r % 64]
    u8 = dict(dtype=torch.uint8, device=dev)
    cap, ctl_cap = 2, 16
    wire = torch.from_numpy(host.reshape(-1)).to(dev)
    dst, ctl = torch.zeros(n * slot, **u8), torch.zeros(n * ctl_cap, **u8)
    frames, msgs = torch.zeros(n * cap * 24, **u8), torch.zeros(n * cap * 32, **u8)
    res, mres = torch.zeros(n * 40, **u8), torch.zeros(n * 64, **u8)
    flows = torch.zeros(n * _lib.MSG_FLOW.itemsize, **u8)
    desc = np.zeros(n, dtype=_lib.MSG_READ)
    regions = np.zeros(n, dtype=_lib.REPLY_REGION)
    for r in range(n):
        desc[r] = (r * slot, r * slot, r * ctl_cap, rlen, r, slot, ctl_cap, r * cap, cap, r * cap, cap, 0)
        regions[r] = (r * oslot, oslot, 0, 0, 0, 0)
    reads = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    d_regions = torch.from_numpy(regions.view(np.uint8).copy()).to(dev)
    ctx = gpu.Ctx(0)
    s = torch.cuda.current_stream()
    pctx = []
    for _ in range(2):
        h = C.c_void_p()
        assert P.fws_gpu_ctx_create(0, C.byref(h)) == 0
        pctx.append(h)
    max_len = rlen
    assert gpu.decode_messages_flow(ctx, wire, reads, n, max_len, frames, msgs, dst, ctl, res, mres, flows, n) == 0
    torch.cuda.synchronize()
    # A CLOSE answered sets close_sent and the next call on that state is silent, so every launch of a measurement
    # gets a fresh state array out of a pool (all forms alike; zeroed outside the timed launches).
    ssz, pool = n * _lib.REPLY_STATE.itemsize, steps + 10
    states = torch.zeros(pool * ssz, **u8)
    both = _lib.FWS_REPLY_CONTROL | _lib.FWS_REPLY_ECHO
    ptr = [t.data_ptr() for t in (reads, msgs, dst, ctl, mres, d_regions, flows)]

    # the timed launches of every form write into one set of buffers, so that where a buffer lies is no difference
    # between the forms; the check before them gives each form its own
    shared = [torch.zeros(n * oslot, **u8), torch.zeros(n * _lib.TX_RESULT.itemsize, **u8),
              torch.zeros(n * _lib.TX_CONN.itemsize, **u8)]

    def form(fn, h, strict, flags=both):
        own = [torch.zeros_like(x) for x in shared]
        k = [0]
        extra = (ptr[6], _lib.MSG_FLOW.itemsize, 0) if strict else ()

        def launch(bufs):
            o, t, c = (x.data_ptr() for x in bufs)
            st = states.data_ptr() + (k[0] % pool) * ssz
            k[0] += 1
            assert fn(h, ptr[0], n, max_len, ptr[1], ptr[2], ptr[3], ptr[4], *extra, ptr[5], o, None, t, c, st, n, flags,
                      s.cuda_stream) == 0

        def measure(steps):
            states.zero_()
            k[0] = 0
            return timed(lambda i: launch(shared), steps)
        return dict(f=lambda i: launch(own), measure=measure, out=own[0], res=own[1], conns=own[2])

    L = _lib.lib()
    forms = {"k_reply": form(L.fws_gpu_reply_messages_multi, ctx.h, False),
             "k_reply_parent_a": form(P.fws_gpu_reply_messages_multi, pctx[0], False),
             "k_reply_parent_b": form(P.fws_gpu_reply_messages_multi, pctx[1], False),
             "k_reply_strict": form(L.fws_gpu_reply_messages_strict, ctx.h, True)}
    strict_parents = ("k_reply_strict_parent_a", "k_reply_strict_parent_b") if parent_has_strict else ()
    forms.update({k: form(P.fws_gpu_reply_messages_strict, h, True) for k, h in zip(strict_parents, pctx)})
    # flags 0: the entries read, the minima, the scan and the table, no frame unless a read fails
    front = {"k_reply_no_frames": form(L.fws_gpu_reply_messages_multi, ctx.h, False, 0),
             "k_reply_strict_no_frames": form(L.fws_gpu_reply_messages_strict, ctx.h, True, 0)}
    # checked first: every form's output, byte for byte
    for v in forms.values():
        states.zero_()
        v["f"](0)
    torch.cuda.synchronize()
    a, st = forms["k_reply"], np.frombuffer(states[:ssz].cpu().numpy().tobytes(), dtype=_lib.REPLY_STATE)
    for k in ("k_reply_parent_a", "k_reply_parent_b") + (() if fail else ("k_reply_strict",)):
        assert all(torch.equal(a[x], forms[k][x]) for x in ("out", "res", "conns")), k
    for k in strict_parents:
        assert all(torch.equal(forms["k_reply_strict"][x], forms[k][x]) for x in ("out", "res", "conns")), k
    t = np.frombuffer(forms["k_reply_strict"]["res"].cpu().numpy().tobytes(), dtype=_lib.TX_RESULT)
    assert (t["status"] == 0).all() and (t["out_len"] == need).all() and (t["n_frames"] == 1).all()
    assert (st["fail_code"] == (1002 if fail else 0)).all() and (st["close_sent"] == int(fail)).all()
    if fail:
        got = forms["k_reply_strict"]["out"].view(n, oslot)[:, :4].cpu().numpy()
        assert (got == np.frombuffer(bytes.fromhex("880203EA"), dtype=np.uint8)).all()
    out = {"measure": "reply_strict", "n": n, "part_bytes": size, "every_read_fails": bool(fail),
           "form": "small" if rlen <= (16 << 10) else "full", "reply_bytes": n * need, "rounds": rounds, "steps": steps,
           "device": torch.cuda.get_device_name(0), "parent_lib": os.path.basename(parent_lib)}
    forms.update(front)
    times = {k: [] for k in forms}
    for rnd in range(rounds):
        for k in (list(forms) if rnd % 2 == 0 else list(forms)[::-1]):
            times[k].append(forms[k]["measure"](steps))
    for k in forms:
        out[k + "_us"] = round(statistics.median(times[k]), 2)
        out[k + "_us_min_max"] = [round(min(times[k]), 2), round(max(times[k]), 2)]
    parent = min(out["k_reply_parent_a_us"], out["k_reply_parent_b_us"])
    out["k_aa_spread_us"] = round(abs(out["k_reply_parent_a_us"] - out["k_reply_parent_b_us"]), 2)
    out["k_reply_minus_parent_us"] = round(out["k_reply_us"] - parent, 2)
    out["k_strict_minus_reply_us"] = round(out["k_reply_strict_us"] - out["k_reply_us"], 2)
    if parent_has_strict:
        sp = [out[k + "_us"] for k in strict_parents]
        out["k_strict_aa_spread_us"] = round(abs(sp[0] - sp[1]), 2)
        out["k_strict_minus_parent_us"] = round(out["k_reply_strict_us"] - min(sp), 2)
    for h in pctx:
        P.fws_gpu_ctx_destroy(h)
    ctx.close()
    return out


def reply_client_bench(n, size, parent_lib, rounds, steps):
    """--reply-client: see the module docstring. size: the message's payload bytes."""
    dev = torch.device("cuda:0")
    P = C.CDLL(parent_lib)
    for name, res_t, args in _lib.SIGNATURES:
        if hasattr(P, name):
            getattr(P, name).restype, getattr(P, name).argtypes = res_t, args
    assert hasattr(P, "fws_gpu_reply_messages_strict"), "--parent-lib has no reply calls"
    rng = np.random.default_rng(41 * n + size)
    hdr = [header(2, 1, size, int(rng.integers(0, 1 << 32))) for _ in range(min(n, 64))]
    rlen = len(hdr[0]) + size
    slot = (rlen + 15) & ~15
    need = size + (2 if size < 126 else 4 if size <= 65535 else 10)
    oslot = (need + 4 + 15) & ~15                     # (one region size for every form: the masked frame fits)
    host = np.zeros((n, slot), dtype=np.uint8)
    body = rng.integers(0, 256, (min(n, 64), size), dtype=np.uint8)
    for r in range(n):
        host[r, :len(hdr[0])] = np.frombuffer(hdr[r % 64], dtype=np.uint8)
        host[r, len(hdr[0]):rlen] = body[r % 64]
    u8 = dict(dtype=torch.uint8, device=dev)
    cap, ctl_cap = 2, 16
    wire = torch.from_numpy(host.reshape(-1)).to(dev)
    dst, ctl = torch.zeros(n * slot, **u8), torch.zeros(n * ctl_cap, **u8)
    frames, msgs = torch.zeros(n * cap * 24, **u8), torch.zeros(n * cap * 32, **u8)
    res, mres = torch.zeros(n * 40, **u8), torch.zeros(n * 64, **u8)
    flows = torch.zeros(n * _lib.MSG_FLOW.itemsize, **u8)
    desc = np.zeros(n, dtype=_lib.MSG_READ)
    regions = np.zeros(n, dtype=_lib.REPLY_REGION)
    sends = np.zeros(n, dtype=_lib.TX_SEND)
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype("<u4")
    for r in range(n):
        desc[r] = (r * slot, r * slot, r * ctl_cap, rlen, r, slot, ctl_cap, r * cap, cap, r * cap, cap, 0)
        regions[r] = (r * oslot, oslot, 0, 0, 0, 0)
        for k, v in dict(src_off=r * slot, out_off=r * oslot, len=size, out_cap=oslot, conn=r, key=int(keys[r]),
                         frame_type=2, last=1, masked=1).items():
            sends[r][k] = v
    reads = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    d_regions = torch.from_numpy(regions.view(np.uint8).copy()).to(dev)
    d_sends = torch.from_numpy(sends.view(np.uint8).copy()).to(dev)
    d_keys = torch.from_numpy(keys.view(np.uint8).copy()).to(dev)
    ctx = gpu.Ctx(0)
    s = torch.cuda.current_stream()
    pctx = []
    for _ in range(2):
        h = C.c_void_p()
        assert P.fws_gpu_ctx_create(0, C.byref(h)) == 0
        pctx.append(h)
    max_len = rlen
    assert gpu.decode_messages_flow(ctx, wire, reads, n, max_len, frames, msgs, dst, ctl, res, mres, flows, n) == 0
    torch.cuda.synchronize()
    echo = _lib.FWS_REPLY_CONTROL | _lib.FWS_REPLY_ECHO
    states = torch.zeros(n * _lib.REPLY_STATE.itemsize, **u8)    # (no CLOSE in the reads: never written)
    ptr = [t.data_ptr() for t in (reads, msgs, dst, ctl, mres, d_regions, flows)]
    # the timed launches of every form write into one set of buffers; the check before them gives each its own
    shared = [torch.zeros(n * oslot, **u8), torch.zeros(n * _lib.TX_RESULT.itemsize, **u8),
              torch.zeros(n * _lib.TX_CONN.itemsize, **u8)]

    def form(fn, h, strict, masked):
        own = [torch.zeros_like(x) for x in shared]
        extra = (ptr[6], _lib.MSG_FLOW.itemsize, 0) if strict else ()
        kp = (d_keys.data_ptr(),) if masked else ()

        def launch(bufs):
            o, t, c = (x.data_ptr() for x in bufs)
            assert fn(h, ptr[0], n, max_len, ptr[1], ptr[2], ptr[3], ptr[4], *extra, ptr[5], o, None, t, c,
                      states.data_ptr(), n, echo, *kp, s.cuda_stream) == 0
        return dict(f=lambda i: launch(own), timed=lambda i: launch(shared), out=own[0], res=own[1], conns=own[2])

    def tx_form():
        own = [torch.zeros_like(x) for x in shared]

        def launch(bufs):
            o, t, c = (x.data_ptr() for x in bufs)
            assert L.fws_gpu_encode_messages_multi(ctx.h, o, ptr[2], d_sends.data_ptr(), n, size, None, t, c, n,
                                                   s.cuda_stream) == 0
        return dict(f=lambda i: launch(own), timed=lambda i: launch(shared), out=own[0], res=own[1], conns=own[2])

    L = _lib.lib()
    forms = {"k_reply": form(L.fws_gpu_reply_messages_multi, ctx.h, False, False),
             "k_reply_parent_a": form(P.fws_gpu_reply_messages_multi, pctx[0], False, False),
             "k_reply_parent_b": form(P.fws_gpu_reply_messages_multi, pctx[1], False, False),
             "k_reply_strict": form(L.fws_gpu_reply_messages_strict, ctx.h, True, False),
             "k_reply_strict_parent_a": form(P.fws_gpu_reply_messages_strict, pctx[0], True, False),
             "k_reply_strict_parent_b": form(P.fws_gpu_reply_messages_strict, pctx[1], True, False),
             "k_reply_client": form(L.fws_gpu_reply_messages_multi_client, ctx.h, False, True),
             "k_reply_strict_client": form(L.fws_gpu_reply_messages_strict_client, ctx.h, True, True),
             "k_tx_multi_masked": tx_form()}
    for v in forms.values():                          # checked first: every form's output, byte for byte
        v["f"](0)
    torch.cuda.synchronize()
    for a, others in (("k_reply", ("k_reply_parent_a", "k_reply_parent_b", "k_reply_strict", "k_reply_strict_parent_a",
                                   "k_reply_strict_parent_b")),
                      ("k_reply_client", ("k_reply_strict_client", "k_tx_multi_masked"))):
        for k in others:
            assert all(torch.equal(forms[a][x], forms[k][x]) for x in ("out", "res", "conns")), k
    for k, want in (("k_reply", need), ("k_reply_client", need + 4)):
        t = np.frombuffer(forms[k]["res"].cpu().numpy().tobytes(), dtype=_lib.TX_RESULT)
        assert (t["status"] == 0).all() and (t["out_len"] == want).all() and (t["n_frames"] == 1).all(), k
    out = {"measure": "reply_client", "n": n, "part_bytes": size, "form": "small" if rlen <= (16 << 10) else "full",
           "reply_bytes": n * need, "reply_bytes_masked": n * (need + 4), "rounds": rounds, "steps": steps,
           "device": torch.cuda.get_device_name(0), "parent_lib": os.path.basename(parent_lib)}
    times = {k: [] for k in forms}
    for rnd in range(rounds):
        for k in (list(forms) if rnd % 2 == 0 else list(forms)[::-1]):
            times[k].append(timed(forms[k]["timed"], steps))
    for k in forms:
        out[k + "_us"] = round(statistics.median(times[k]), 2)
        out[k + "_us_min_max"] = [round(min(times[k]), 2), round(max(times[k]), 2)]
    for k in ("k_reply", "k_reply_strict"):           # the server instantiations against the parent's
        pa, pb = out[k + "_parent_a_us"], out[k + "_parent_b_us"]
        out[k + "_aa_spread_us"] = round(abs(pa - pb), 2)
        out[k + "_minus_parent_us"] = round(out[k + "_us"] - min(pa, pb), 2)
        out[k + "_within_twice_the_spread"] = bool(out[k + "_us"] - min(pa, pb) <= 2 * abs(pa - pb))
    out["masked_over_unmasked"] = round(out["k_reply_client_us"] / out["k_reply_us"], 3)
    out["strict_masked_over_unmasked"] = round(out["k_reply_strict_client_us"] / out["k_reply_strict_us"], 3)
    out["masked_over_tx_multi_masked"] = round(out["k_reply_client_us"] / out["k_tx_multi_masked_us"], 3)
    out["k_reply_gb_s"] = round(n * need / out["k_reply_us"] / 1e3, 2)
    out["k_reply_client_gb_s"] = round(n * (need + 4) / out["k_reply_client_us"] / 1e3, 2)
    out["k_tx_multi_masked_gb_s"] = round(n * (need + 4) / out["k_tx_multi_masked_us"] / 1e3, 2)
    for h in pctx:
        P.fws_gpu_ctx_destroy(h)
    ctx.close()
    return out


def client_read(wire):
    """A read of whole masked frames as a server writes it: the same payloads, no MASK bit, no key."""
    out, pos = bytearray(), 0
    while pos < len(wire):
        b1 = wire[pos + 1]
        assert b1 & 0x80
        n, h = b1 & 127, 2
        if n == 126:
            n, h = struct.unpack(">H", wire[pos + 2:pos + 4])[0], 4
        elif n == 127:
            n, h = struct.unpack(">Q", wire[pos + 2:pos + 10])[0], 10
        key = np.frombuffer(wire[pos + h:pos + h + 4], dtype=np.uint8)
        body = np.frombuffer(wire[pos + h + 4:pos + h + 4 + n], dtype=np.uint8) ^ np.resize(key, n)
        out += bytes([wire[pos], b1 & 0x7F]) + wire[pos + 2:pos + h] + body.tobytes()
        pos += h + 4 + n
    assert pos == len(wire)
    return bytes(out)


def flow_client_bench(n, size, parent_lib, rounds, steps):
    """--flow-client: see the module docstring."""
    dev = torch.device("cuda:0")
    P = C.CDLL(parent_lib)
    for name, res_t, args in _lib.SIGNATURES:
        if hasattr(P, name):
            getattr(P, name).restype, getattr(P, name).argtypes = res_t, args
    assert hasattr(P, "fws_gpu_decode_messages_flow"), "--parent-lib has no flow call"
    rng = np.random.default_rng(1000 * n + size)
    distinct = [multi_read(rng, size) for _ in range(min(n, 64))]
    cap = max(f for _, f in distinct) + 4
    ctl_cap = 8 * (cap // 64 + 2)
    unmasked = [client_read(w) for w, _ in distinct]
    host = np.stack([np.frombuffer(w, dtype=np.uint8) for w, _ in distinct])
    chost = np.zeros_like(host)
    for i, w in enumerate(unmasked):
        chost[i, :len(w)] = np.frombuffer(w, dtype=np.uint8)
    pick = np.arange(n) % len(distinct)
    u8 = dict(dtype=torch.uint8, device=dev)
    wire, cwire = torch.from_numpy(host[pick].reshape(-1)).to(dev), torch.from_numpy(chost[pick].reshape(-1)).to(dev)
    dst, ctl = torch.zeros(n * size, **u8), torch.zeros(n * ctl_cap, **u8)
    frames, msgs = torch.zeros(n * cap * 24, **u8), torch.zeros(n * cap * 32, **u8)
    res, mres = torch.zeros(n * 40, **u8), torch.zeros(n * 64, **u8)
    flows = torch.zeros(n * _lib.MSG_FLOW.itemsize, **u8)
    desc, cdesc = np.zeros(n, dtype=_lib.MSG_READ), np.zeros(n, dtype=_lib.MSG_READ)
    for r in range(n):
        desc[r] = (r * size, r * size, r * ctl_cap, size, r, size, ctl_cap, r * cap, cap, r * cap, cap, 0)
        cdesc[r] = desc[r]
        cdesc[r]["len"] = len(unmasked[pick[r]])
    reads = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    creads = torch.from_numpy(cdesc.view(np.uint8).copy()).to(dev)
    ctx = gpu.Ctx(0)
    s = torch.cuda.current_stream()
    pctx = []
    for _ in range(2):
        h = C.c_void_p()
        assert P.fws_gpu_ctx_create(0, C.byref(h)) == 0
        pctx.append(h)

    def form(h, fn, w, rd):
        def f(i):
            assert fn(h, w.data_ptr(), rd.data_ptr(), n, size, frames.data_ptr(), msgs.data_ptr(), dst.data_ptr(),
                      ctl.data_ptr(), res.data_ptr(), mres.data_ptr(), flows.data_ptr(), n, s.cuda_stream) == 0
        return f

    L = _lib.lib()
    forms = {"flow_parent_a": form(pctx[0], P.fws_gpu_decode_messages_flow, wire, reads),
             "flow_parent_b": form(pctx[1], P.fws_gpu_decode_messages_flow, wire, reads),
             "flow": form(ctx.h, L.fws_gpu_decode_messages_flow, wire, reads),
             "flow_client": form(ctx.h, L.fws_gpu_decode_messages_flow_client, cwire, creads)}
    want = None
    for k, f in forms.items():                        # checked first
        for t in (dst, ctl, frames, msgs, res, mres, flows):
            t.zero_()
        f(0)
        torch.cuda.synchronize()
        m = np.frombuffer(mres.cpu().numpy().tobytes(), dtype=_lib.MSG_RESULT).copy()
        assert (m["status"] == 0).all() and (m["open_opcode"] == 0).all(), k
        assert (m["resume_off"] == (cdesc["len"] if k == "flow_client" else size)).all(), k
        m["resume_off"] = 0
        # the server forms: every byte; the client: the bytes, the control payloads, the entries and the results
        got = [t.clone() for t in (dst, ctl, msgs)] + [m.tobytes()]
        got += [] if k == "flow_client" else [t.clone() for t in (frames, res, flows)]
        want = want or got
        for a, b in zip(got, want):
            assert torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b, k
    times = {k: [] for k in forms}
    for rnd in range(rounds):
        for k in (list(forms) if rnd % 2 == 0 else list(forms)[::-1]):
            times[k].append(timed(forms[k], steps))
    out = {"measure": "flow_client", "n": n, "read_bytes": size, "form": "small" if size <= (16 << 10) else "full",
           "wire_bytes": n * size, "client_wire_bytes": int(cdesc["len"].astype(np.int64).sum()), "rounds": rounds,
           "steps": steps, "device": torch.cuda.get_device_name(0), "parent_lib": os.path.basename(parent_lib)}
    for k in forms:
        out[k + "_us"] = round(statistics.median(times[k]), 2)
        out[k + "_us_min_max"] = [round(min(times[k]), 2), round(max(times[k]), 2)]
    base = min(out["flow_parent_a_us"], out["flow_parent_b_us"])
    out["flow_aa_spread_us"] = round(abs(out["flow_parent_a_us"] - out["flow_parent_b_us"]), 2)
    out["flow_minus_parent_us"] = round(out["flow_us"] - base, 2)
    out["flow_within_twice_the_spread"] = bool(out["flow_us"] - base <= 2 * out["flow_aa_spread_us"])
    out["client_over_server"] = round(out["flow_client_us"] / out["flow_us"], 3)
    for h in pctx:
        P.fws_gpu_ctx_destroy(h)
    ctx.close()
    return out


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
    ap.add_argument("--carry", action="store_true", help="measure fws_gpu_decode_messages_carry (see above)")
    ap.add_argument("--parent-lib", default="", help="libfws_gpu.so built from the parent commit, for (i)")
    ap.add_argument("--read-mib", type=float, default=2.0)
    ap.add_argument("--multi", action="store_true", help="measure fws_gpu_decode_messages_multi (see above)")
    ap.add_argument("--grid-n", default="1,8,64,512,4096", help="--multi: connections")
    ap.add_argument("--grid-kib", default="1,4,16,64", help="--multi: read sizes, KiB")
    ap.add_argument("--flow", action="store_true", help="measure fws_gpu_decode_messages_flow (see above)")
    ap.add_argument("--flow-conns", type=int, default=64, help="--flow (ii): connections")
    ap.add_argument("--flow-frame-kib", type=int, default=1024, help="--flow (ii): a frame on the wire, KiB")
    ap.add_argument("--flow-read-kib", type=int, default=16, help="--flow (ii): a read, KiB")
    ap.add_argument("--tx-multi", action="store_true", help="measure fws_gpu_encode_messages_multi (see above)")
    ap.add_argument("--reply", action="store_true", help="measure fws_gpu_reply_messages_multi (see above)")
    ap.add_argument("--reply-strict", action="store_true",
                    help="measure fws_gpu_reply_messages_strict against the plain call and the parent's (see above)")
    ap.add_argument("--reply-client", action="store_true",
                    help="measure the masked (client) reply calls and the server calls against the parent's (see above)")
    ap.add_argument("--flow-client", action="store_true",
                    help="measure fws_gpu_decode_messages_flow_client and the server call against the parent's")
    ap.add_argument("--join", action="store_true", help="measure fws_gpu_join_messages (see above)")
    ap.add_argument("--publish", action="store_true", help="measure fws_gpu_publish_messages (see above)")
    ap.add_argument("--cases", default="a,b,c,d", help="--publish: the cases to run")
    a = ap.parse_args()
    target = a.target << 20
    lines = []
    if a.publish:
        for case in a.cases.split(","):
            lines.append(json.dumps(publish_bench(case, os.path.abspath(a.parent_lib) if a.parent_lib else "",
                                                  a.rounds, max(a.steps, 100))))
            print(lines[-1], flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    if a.join:
        assert a.parent_lib, "--join needs --parent-lib"
        grid_n = "64,512,4096" if a.grid_n == ap.get_default("grid_n") else a.grid_n
        grid_kib = "4,64" if a.grid_kib == ap.get_default("grid_kib") else a.grid_kib
        for kib in map(int, grid_kib.split(",")):
            for n in map(int, grid_n.split(",")):
                lines.append(json.dumps(join_bench(n, kib << 10, os.path.abspath(a.parent_lib), a.rounds, a.steps,
                                                   loop=kib == 4)))
                print(lines[-1], flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    if a.reply_client or a.flow_client:
        assert a.parent_lib, "--reply-client / --flow-client need --parent-lib"
        lib = os.path.abspath(a.parent_lib)
        if a.reply_client:
            for n, kib in ((64, 4), (512, 4), (4096, 4), (64, 64), (512, 64)):
                lines.append(json.dumps(reply_client_bench(n, kib << 10, lib, a.rounds, a.steps)))
                print(lines[-1], flush=True)
        else:
            grid_n = "1,64,512" if a.grid_n == ap.get_default("grid_n") else a.grid_n
            for kib in map(int, a.grid_kib.split(",")):
                for n in map(int, grid_n.split(",")):
                    lines.append(json.dumps(flow_client_bench(n, kib << 10, lib, a.rounds, a.steps)))
                    print(lines[-1], flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    if a.reply_strict:
        assert a.parent_lib, "--reply-strict needs --parent-lib"
        lib = os.path.abspath(a.parent_lib)
        for n, kib, fail in ((64, 4, False), (512, 4, False), (4096, 4, False), (512, 64, False), (512, 0, True)):
            lines.append(json.dumps(reply_strict_bench(n, kib << 10, lib, a.rounds, a.steps, fail=fail)))
            print(lines[-1], flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    if a.reply:
        assert a.parent_lib, "--reply needs --parent-lib"
        grid_n = "64,512,4096" if a.grid_n == ap.get_default("grid_n") else a.grid_n
        grid_kib = "4,64" if a.grid_kib == ap.get_default("grid_kib") else a.grid_kib
        for kib in map(int, grid_kib.split(",")):
            for n in map(int, grid_n.split(",")):
                if n * (kib << 10) > (64 << 20):          # (the kernel comparison at 64 KiB: up to 1024 connections)
                    continue
                lines.append(json.dumps(reply_bench(n, kib << 10, os.path.abspath(a.parent_lib), a.rounds, a.steps,
                                                    loop=kib == 4)))
                print(lines[-1], flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    if a.tx_multi:
        grid_n = "1,64,512" if a.grid_n == ap.get_default("grid_n") else a.grid_n
        points = [(n, kib << 10, 0) for kib in map(int, a.grid_kib.split(",")) for n in map(int, grid_n.split(","))]
        for n, size, mf in points + [(64, 64 << 10, 4096)]:
            lines.append(json.dumps(tx_multi_bench(n, size, mf, a.rounds, a.steps)))
            print(lines[-1], flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    if a.flow:
        if a.parent_lib:
            grid_n = "1,64,512" if a.grid_n == ap.get_default("grid_n") else a.grid_n
            for kib in map(int, a.grid_kib.split(",")):
                for n in map(int, grid_n.split(",")):
                    lines.append(json.dumps(flow_cost(n, kib << 10, os.path.abspath(a.parent_lib), a.rounds, a.steps)))
                    print(lines[-1], flush=True)
        lines.append(json.dumps(flow_frames(a.flow_conns, a.flow_frame_kib << 10, a.flow_read_kib << 10, a.rounds)))
        print(lines[-1], flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    if a.multi:
        for kib in map(int, a.grid_kib.split(",")):
            for n in map(int, a.grid_n.split(",")):
                lines.append(json.dumps(multi_bench(n, kib << 10, a.rounds, a.steps)))
                print(lines[-1], flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    if a.carry:
        wire, _, _, n_frames = fragmented_stream(target)
        if a.parent_lib:
            lines.append(json.dumps(carry_cost(wire, n_frames, os.path.abspath(a.parent_lib), a.rounds, a.steps)))
            print(lines[-1], flush=True)
        for name, w in (("frag", wire), ("one_message_64k", one_message_stream(target))):
            lines.append(json.dumps(carry_reads(name, w, int(a.read_mib * (1 << 20)), a.rounds)))
            print(lines[-1], flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
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
