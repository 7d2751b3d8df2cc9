"""Cost of the request-address kernels (hysteria_amd/csrc/addr.hip) on one GPU: for
each of two mixes of N addresses,

  parse    hyobfs_addr_parse_batch over the N texts, packed back to back
  match    hyobfs_acl_match_batch alone over what that call left (the same names,
           addresses and ports) with a small rule set, so the cost the parse adds to
           the chain is visible next to the call it feeds
  format   hyobfs_addr_format_batch (48-byte rows, with meta) over the mix's addresses

every timing the median of per-step HIP event times after warm-up, and next to them,
in a process of its own and before this one opens the GPU,

  host     tools/addr_host_bench.cpp: the scalar host ABI (hyobfs_addr_parse,
           hyobfs_addr_format) on 16 threads over the same items

The mixes: "v4_90" is 90 % IPv4 literals and 10 % domains; "thirds" is equal thirds
of IPv4 literals, bracketed IPv6 literals and domains.  Ports are uniform in
[1, 65535]; the format leg's addresses are the mix's literals, the domains' share
becoming IPv4 addresses.  The tool is built with the machine's compiler if its
binary is missing (tools/addr_host_bench; it is not kept in git).

Prints one JSON line.

  python scripts/bench_addr.py [--n 1048576] [--steps 50] [--warmup 5] [--out FILE]
"""
import argparse
import ipaddress
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POOL = 1 << 16   # distinct texts per kind; every item still has bytes of its own in the buffer
RULES = "pinned(1.2.3.4)\nlan(10.0.0.0/8)\nsite(suffix:example.com)\nreject(suffix:bad.test)\ngames(all, udp/1000-2000)\n"
OUTBOUNDS = {"pinned": 1, "lan": 2, "site": 3, "reject": 4, "games": 5}


def _pool(rng):
    """Per kind (0 IPv4, 1 bracketed IPv6, 2 domain): POOL host texts and their 16-byte addresses."""
    v4 = rng.integers(0, 256, (POOL, 4), dtype=np.uint8)
    v6 = rng.integers(0, 256, (POOL, 16), dtype=np.uint8)
    v6[rng.random((POOL, 16)) < 0.4] = 0   # zero bytes, so that "::" and short groups occur
    v6[:, 0] = 0x20
    labels = [b"www", b"api", b"cdn", b"mail", b"edge-7", b"static", b"a", b"video-cache"]
    tlds = [b"example.com", b"example.org", b"bad.test", b"service.internal", b"co.uk"]
    hosts = [[b"%d.%d.%d.%d" % tuple(r) for r in v4],
             [b"[" + str(ipaddress.IPv6Address(bytes(r))).encode() + b"]" for r in v6],
             [labels[i % 8] + b"%d." % (i * 7919 % 100000) + tlds[i % 5] for i in range(POOL)]]
    ip16 = [np.concatenate([np.zeros((POOL, 10), np.uint8), np.full((POOL, 2), 255, np.uint8), v4], 1), v6]
    return hosts, ip16


def make_mix(name, n, seed):
    rng = np.random.default_rng(seed)
    hosts, ip16 = _pool(rng)
    u = rng.random(n)
    kind = np.where(u < 0.9, 0, 2) if name == "v4_90" else np.minimum((u * 3).astype(np.int64), 2)
    pick = rng.integers(0, POOL, n)
    port = rng.integers(1, 65536, n).astype(np.uint16)
    # the pool's texts "host:" + the port in decimal, gathered into one buffer
    pool_txt = [h + b":" for k in range(3) for h in hosts[k]]
    pool_len = np.array([len(t) for t in pool_txt], np.int64)
    pool_off = np.concatenate([[0], np.cumsum(pool_len)[:-1]])
    pool_buf = np.frombuffer(b"".join(pool_txt), np.uint8)
    pid = kind * POOL + pick
    digits = np.char.encode(port.astype("U5"))   # S5, right-padded with NUL
    dlen = np.char.str_len(digits).astype(np.int64)
    hlen = pool_len[pid]
    lens = hlen + dlen
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    buf = np.zeros(int(lens.sum()) + 16, np.uint8)
    hpos = np.arange(int(hlen.sum())) - np.repeat(np.cumsum(hlen) - hlen, hlen)
    buf[np.repeat(off, hlen) + hpos] = pool_buf[np.repeat(pool_off[pid], hlen) + hpos]
    dmat = np.frombuffer(digits.tobytes(), np.uint8).reshape(n, -1)
    for c in range(dmat.shape[1]):
        m = dlen > c
        buf[off[m] + hlen[m] + c] = dmat[m, c]
    fam = np.where(kind == 1, 16, 4).astype(np.uint8)
    ip = np.where((kind == 1)[:, None], ip16[1][pick], 0).astype(np.uint8)
    ip[kind != 1, :4] = ip16[0][pick[kind != 1], 12:]
    return {"buf": buf, "off": off.astype(np.uint64), "len": lens.astype(np.uint32), "ip": ip.reshape(-1), "family": fam,
            "port": port, "kinds": [int((kind == k).sum()) for k in range(3)]}


def host_leg(mix, threads):
    exe = os.path.join(ROOT, "tools", "addr_host_bench")
    if not os.path.exists(exe):
        subprocess.run(["g++", "-O2", "-std=c++17", "tools/addr_host_bench.cpp", "-ldl", "-lpthread", "-o", exe], check=True,
                       cwd=ROOT)
    with tempfile.NamedTemporaryFile(suffix=".bin") as f:
        n = len(mix["off"])
        f.write(np.array([n, len(mix["buf"])], np.uint64).tobytes())
        for k in ("off", "len", "buf", "ip", "family", "port"):
            f.write(mix[k].tobytes())
        f.flush()
        out = subprocess.run([exe, os.path.join(ROOT, "hysteria_amd", "libhyobfs.so"), f.name, str(threads), "5"], check=True,
                             capture_output=True, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])


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
    return {"ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "per_s": round(n / med * 1e3),
            "ns_per_item": round(med * 1e6 / n, 3), **more}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--no-host-leg", action="store_true", help="the device legs only")
    a = ap.parse_args()
    mixes = {name: make_mix(name, a.n, seed) for name, seed in (("v4_90", 11), ("thirds", 12))}
    host = {} if a.no_host_leg else {name: host_leg(m, a.host_threads) for name, m in mixes.items()}
    import torch

    import hysteria_amd
    from hysteria_amd import acl, addr, udpmsg
    if not torch.cuda.is_available():
        raise SystemExit("bench_addr.py needs a GPU: nothing is measured without one")
    dev, n = torch.device("cuda", 0), a.n
    res = {"n": n, "steps": a.steps, "warmup": a.warmup, "build_id": hysteria_amd.build_id(),
           "device": torch.cuda.get_device_name(0), "rules": len(OUTBOUNDS)}
    with hysteria_amd.compile_rules(hysteria_amd.parse_text_rules(RULES), OUTBOUNDS) as rs:
        for name, m in mixes.items():
            t = {k: torch.from_numpy(v.view(np.int16) if v.dtype == np.uint16 else v.view(np.int64) if v.dtype == np.uint64
                                     else v.view(np.int32) if v.dtype == np.uint32 else v).to(dev) for k, v in m.items()
                 if k != "kinds"}
            st, noff, nlen, v4, v6, fl, port = addr.parse_outputs(n, dev)
            r = {"kinds": m["kinds"], "text_bytes": int(m["len"].sum())}
            r["parse"] = leg(n, timed(torch, lambda: addr.parse_batch(t["buf"], t["off"], t["len"], n, st, noff, nlen, v4, v6, fl,
                                                                      port), a.steps, a.warmup))
            assert not st.any() and int((fl != 0).sum()) == m["kinds"][0] + m["kinds"][1]
            assert torch.equal(port, t["port"])
            proto = torch.full((n,), acl.PROTO_UDP, dtype=torch.uint8, device=dev)
            d_res = torch.zeros(n * acl.ACL_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            r["match"] = leg(n, timed(torch, lambda: rs.match_batch(t["buf"], noff, nlen, v4, v6, fl, proto, port, n, d_res),
                                      a.steps, a.warmup))
            r["parse_over_match"] = round(r["parse"]["ms"] / r["match"]["ms"], 3)
            stride = 48
            rows = torch.empty(n * stride, dtype=torch.uint8, device=dev)
            olen = torch.empty(n, dtype=torch.int32, device=dev)
            fst = torch.empty(n, dtype=torch.int32, device=dev)
            meta = torch.zeros(n * udpmsg.META_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            r["format"] = leg(n, timed(torch, lambda: addr.format_batch(t["ip"], t["family"], t["port"], n, rows, stride, 0, olen,
                                                                        meta, fst), a.steps, a.warmup),
                              out_stride=stride, text_bytes=int(olen.sum().item()))
            assert not fst.any()
            # what was formatted parses back to the same ports
            foff = torch.arange(n, dtype=torch.int64, device=dev) * stride
            addr.parse_batch(rows, foff, olen, n, st, noff, nlen, v4, v6, fl, port)
            assert not st.any() and torch.equal(port, t["port"])
            if name in host:
                r["host"] = host[name]
            res[name] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
