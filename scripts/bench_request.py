"""Cost of the request-hook kernels (hysteria_amd/csrc/request.hip) on one GPU over N
new TCP streams, every kernel timing the median of per-step HIP event times after
warm-up:

  parse      hyobfs_tcp_request_parse_batch over the N stream prefixes
  check      hyobfs_sniff_check_batch over the addresses that call found (RewriteDomain
             off, a port set of three ranges)
  rewrite    hyobfs_request_rewrite_batch with what hyobfs_tcp_sniff_batch found behind the
             requests (that call is run once and is not timed here), 320-byte rows
  response   hyobfs_tcp_response_build_batch: N rows of 1280 bytes, padding lengths uniform
             in [128, 1024) (tcpResponsePadding), three messages; bytes/s of what it writes
  pipeline   hysteria_amd.tcp_request_decisions over the same streams as host byte strings:
             wall time of the whole call (packing, the copies to and from the device and
             the per-stream Python results included), the median of `--pipeline-steps` runs

and two yardsticks for the response kernel, which only stores:

  row_copy    a device-to-device copy (torch) of N rows of the mean response length into
              the same strided output: the same output shape, nothing computed
  copy_probe  tools/bimodal_copy.hip, the copy probe of scripts/bench_udpmsg.py, in a
              process of its own before this one opens the GPU: N packed datagrams of 64 /
              1350 bytes; its best variant's rate (bytes read + written, so halve it to
              compare stores with stores)

The streams: 90 % IPv4 literals and 10 % domains, ports 80 / 443 / 8080 / random; behind
the request a TLS ClientHello record with a server name (1/2), an HTTP request (1/4) or
bytes of neither (1/4); request padding uniform in [64, 512) (tcpRequestPadding).

Prints one JSON line.

  python scripts/bench_request.py [--n 1048576] [--steps 30] [--warmup 5] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POOL = 1 << 12   # distinct stream prefixes; every item still has bytes of its own in the buffer
RULES = "pinned(1.2.3.4)\nlan(10.0.0.0/8)\nsite(suffix:example.com)\nreject(suffix:bad.test)\ngames(all, udp/1000-2000)\n"
OUTBOUNDS = {"pinned": 1, "lan": 2, "site": 3, "reject": 4, "games": 5}
TCP_PORTS = [(80, 80), (443, 443), (8000, 8999)]
ROW, RESP_ROW = 320, 1280


def _varint(v):
    return bytes([v]) if v < 64 else (0x4000 | v).to_bytes(2, "big")


def _hello(name: bytes) -> bytes:
    """A TLS record that holds a ClientHello with a server_name extension."""
    sni = (len(name) + 3).to_bytes(2, "big") + b"\x00" + len(name).to_bytes(2, "big") + name
    exts = b"\x00\x0a\x00\x04\x00\x02\x00\x1d" + b"\x00\x00" + len(sni).to_bytes(2, "big") + sni + b"\x00\x2b\x00\x03\x02\x03\x04"
    body = (b"\x03\x03" + bytes(range(32)) + b"\x20" + bytes(32) + b"\x00\x04\x13\x01\x13\x02" + b"\x01\x00"
            + len(exts).to_bytes(2, "big") + exts)
    msg = b"\x01" + len(body).to_bytes(3, "big") + body
    return b"\x16\x03\x01" + len(msg).to_bytes(2, "big") + msg


def make_pool(rng):
    labels = [b"www", b"api", b"cdn", b"mail", b"edge-7", b"static", b"a", b"video-cache"]
    tlds = [b"example.com", b"example.org", b"bad.test", b"service.internal", b"co.uk"]
    pool = []
    for i in range(POOL):
        name = labels[i % 8] + b"%d." % (i * 7919 % 100000) + tlds[i % 5]
        port = (b"80", b"443", b"8080", b"%d" % rng.integers(1, 65536))[i % 4]
        host = name if i % 10 == 9 else b"%d.%d.%d.%d" % tuple(rng.integers(1, 255, 4))
        addr = host + b":" + port
        kind = i % 4
        payload = (_hello(name) if kind < 2 else b"GET /index.html HTTP/1.1\r\nHost: " + name + b"\r\nAccept: */*\r\n\r\n"
                   if kind == 2 else b"\x00\x01\x02" + bytes(rng.integers(0, 256, 48, dtype=np.uint8)))
        pad = int(rng.integers(64, 512))
        pool.append(_varint(len(addr)) + addr + _varint(pad) + b"p" * pad + payload)
    return pool


def probe_leg(n):
    exe = os.path.join(ROOT, "tools", "bimodal_copy")
    if not os.path.exists(exe):
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "tools/bimodal_copy.hip", "-o", exe], check=True,
                       cwd=ROOT)
    out = subprocess.run([exe, str(n)], check=True, capture_output=True, text=True).stdout
    r = json.loads(out[out.index("{"):])
    best = max(r["results"], key=lambda x: x["GBs"])
    return {"n": r["n"], "algorithmic_bytes": r["algorithmic_bytes"], "output_bytes": r["output_bytes"], "best": best}


def timed(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def leg(n, t, **more):
    med, lo, hi = t
    return {"ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "items_per_s": round(n / med * 1e3), **more}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pipeline-steps", type=int, default=3)
    ap.add_argument("--no-side-legs", action="store_true", help="without the copy probe's process")
    ap.add_argument("--out")
    a = ap.parse_args()
    side = {} if a.no_side_legs else {"copy_probe": probe_leg(a.n)}
    import torch

    import hysteria_amd
    from hysteria_amd import request, sniff
    if not torch.cuda.is_available():
        raise SystemExit("bench_request.py needs a GPU: nothing is measured without one")
    dev, n = torch.device("cuda", 0), a.n
    rng = np.random.default_rng(0x4E9)
    pool = make_pool(rng)
    pick = rng.integers(0, POOL, n)
    streams = [pool[i] for i in pick]
    lens = np.array([len(s) for s in streams], np.uint32)
    off = np.zeros(n, np.uint64)
    np.cumsum(lens[:-1], out=off[1:])
    d_in = torch.from_numpy(np.frombuffer(b"".join(streams) + bytes(16), np.uint8).copy()).to(dev)
    d_off, d_len = torch.from_numpy(off).to(dev), torch.from_numpy(lens).to(dev)
    i32 = lambda k=n: torch.zeros(k, dtype=torch.int32, device=dev)   # noqa: E731
    i64 = lambda: torch.zeros(n, dtype=torch.int64, device=dev)   # noqa: E731
    u8 = lambda k=n: torch.zeros(k, dtype=torch.uint8, device=dev)   # noqa: E731
    res = {"n": n, "stream_bytes": int(lens.sum()), "steps": a.steps, "warmup": a.warmup, "build_id": hysteria_amd.build_id(),
           "device": torch.cuda.get_device_name(0)}

    st, need, aoff, alen, roff, rlen = i32(), i32(), i64(), i32(), i64(), i32()
    res["parse"] = leg(n, timed(torch, lambda: request.tcp_request_parse_batch(d_in, d_off, d_len, n, st, need, aoff, alen, roff,
                                                                               rlen), a.steps, a.warmup))
    assert int((st != 0).sum()) == 0

    chk = u8()
    with request.PortSet(TCP_PORTS) as ports:
        res["check"] = leg(n, timed(torch, lambda: request.sniff_check_batch(d_in, aoff, alen, st, n, False, False, ports, chk),
                                    a.steps, a.warmup), checked=int(chk.sum()))

    names, sres = u8(n * 255), u8(n * 16)
    sniff.tcp_sniff_batch(d_in, roff, rlen, n, names, 255, sres)
    rows, rowoff, outlen, rew, rst = u8(n * ROW), i64(), i32(), u8(), i32()
    res["rewrite"] = leg(n, timed(torch, lambda: request.request_rewrite_batch(d_in, aoff, alen, st, chk, names, 255, sres, n, rows,
                                                                               ROW, 0, rowoff, outlen, rew, rst), a.steps, a.warmup),
                         rewritten=int(rew.sum()), row_bytes=n * ROW)
    assert int((rst != 0).sum()) == 0
    res["rewrite"]["GB_per_s_written"] = round(n * ROW / res["rewrite"]["ms"] / 1e6, 1)

    msgs = [b"RequestHook enabled", b"Connected", b"connection rejected by the ACL"]
    mbuf = torch.from_numpy(np.frombuffer(b"".join(msgs), np.uint8).copy()).to(dev)
    moff = torch.tensor([0, len(msgs[0]), len(msgs[0]) + len(msgs[1])], dtype=torch.int64, device=dev)
    mlen = torch.tensor([len(m) for m in msgs], dtype=torch.int32, device=dev)
    midx = torch.from_numpy(rng.integers(0, 3, n).astype(np.int32)).to(dev)
    ok = (midx < 2).to(torch.uint8)
    pad = torch.from_numpy(rng.integers(128, 1024, n).astype(np.int32)).to(dev)
    resp, resplen, respst = u8(n * RESP_ROW), i32(), i32()
    t = timed(torch, lambda: request.tcp_response_build_batch(ok, midx, mbuf, moff, mlen, 3, pad, 7, n, resp, RESP_ROW, resplen,
                                                              respst), a.steps, a.warmup)
    written = int(resplen.to(torch.int64).sum())
    assert int((respst != 0).sum()) == 0
    res["response"] = leg(n, t, bytes_written=written, GB_per_s_written=round(written / t[0] / 1e6, 1))
    mean = written // n
    src = torch.empty(n, mean, dtype=torch.uint8, device=dev)
    view = resp.view(n, RESP_ROW)[:, :mean]
    t = timed(torch, lambda: view.copy_(src), a.steps, a.warmup)
    res["row_copy"] = leg(n, t, row_bytes=mean, GB_per_s_written=round(n * mean / t[0] / 1e6, 1))
    res["response"]["ratio_to_row_copy"] = round(res["response"]["GB_per_s_written"] / res["row_copy"]["GB_per_s_written"], 3)
    if side:
        p = side["copy_probe"]
        p["GB_per_s_written"] = round(p["best"]["GBs"] * p["output_bytes"] / p["algorithmic_bytes"], 1)
        res["response"]["ratio_to_copy_probe"] = round(res["response"]["GB_per_s_written"] / p["GB_per_s_written"], 3)
    del src, view, resp, rows, names

    sniffer = hysteria_amd.Sniffer(rewrite_domain=False, tcp_ports=TCP_PORTS)
    secs = []
    with hysteria_amd.compile_rules(hysteria_amd.parse_text_rules(RULES), OUTBOUNDS) as rs:
        for _ in range(1 + a.pipeline_steps):
            t0 = time.perf_counter()
            got = hysteria_amd.tcp_request_decisions(rs, sniffer, streams, refusals={4: "connection rejected by the ACL"}, seed=7,
                                                     out_stride=ROW, resp_stride=RESP_ROW)
            secs.append(time.perf_counter() - t0)
    med = float(np.median(secs[1:]))
    res["pipeline"] = {"s": round(med, 3), "s_min": round(min(secs[1:]), 3), "s_max": round(max(secs[1:]), 3),
                       "items_per_s": round(n / med), "ok": int((got.status == 0).sum()), "checked": int(got.check.sum()),
                       "note": "wall time of the whole Python call, host packing and per-stream results included"}
    res.update(side)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
