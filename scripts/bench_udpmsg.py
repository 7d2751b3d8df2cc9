"""Cost of the UDP relay message kernels (hysteria_amd/csrc/udpmsg.hip) on one GPU,
three legs in one process, every timing the median of per-step HIP event times
after warm-up:

  frag      hyobfs_udp_frag_batch (plan, scan, index and write kernels) over N
            messages: hyobfs_synth_bimodal_lengths data (64 / 1350 bytes), one
            11-byte address, max_size 1200
  parse     hyobfs_udp_parse_batch over the datagrams that leg produced
  assemble  hyobfs_udp_assemble_batch of those datagrams back into the N messages
            (the fragment lists are `first` itself: no host Defragger in the loop)

Next to them, each in a process of its own and before this one opens the GPU:

  host        tools/udpmsg_host_bench.cpp: the scalar host ABI (hyobfs_udp_send_frags,
              hyobfs_udp_parse) on 16 threads over 1M messages of the same mix
  copy_probe  tools/bimodal_copy.hip: the project's copy probe of the bimodal mix
              (contiguous input, packed output, an 8-byte field written in front of every
              payload, nothing computed).  Its byte movement is the frag call's but for the
              header (8 bytes per datagram where a relay message has 20 per fragment) and
              the cut of the 1350-byte payloads into two datagrams; its `wave` variants are
              the shape of the write kernel here (one wave per run of datagrams, 16-byte
              windows, masked edge windows).

Both are built with the compilers of the machine if their binaries are missing
(tools/udpmsg_host_bench, tools/bimodal_copy; they are not kept in git).

Rates: messages/s, GiB/s of payload, and the share of the 8 TB/s HBM peak by
ALGORITHMIC bytes (payload read + datagram bytes written, resp. payload slices
read + message bytes written); the index arrays each call also moves are listed
separately as index_bytes and are not in that share.

Prints one JSON line.

  python scripts/bench_udpmsg.py [--n 4194304] [--steps 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12   # bytes/s, MI355X HBM3E spec
ADDR = b"10.0.0.1:53"


def _tool(exe, build):
    path = os.path.join(ROOT, "tools", exe)
    if not os.path.exists(path):
        subprocess.run(build + ["-o", path], check=True, cwd=ROOT)
    return path


def host_leg(n, threads):
    exe = _tool("udpmsg_host_bench", ["g++", "-O2", "-std=c++17", "tools/udpmsg_host_bench.cpp", "-ldl", "-lpthread"])
    out = subprocess.run([exe, os.path.join(ROOT, "hysteria_amd", "libhyobfs.so"), str(n), str(threads), "5"], check=True,
                         capture_output=True, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def probe_leg(n):
    exe = _tool("bimodal_copy", ["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "tools/bimodal_copy.hip"])
    out = subprocess.run([exe, str(n)], check=True, capture_output=True, text=True).stdout
    return json.loads(out[out.index("{"):])


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


def leg(n, payload, algo, index, t):
    med, lo, hi = t
    return {"ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "msgs_per_s": round(n / med * 1e3),
            "payload_GiB_per_s": round(payload / med * 1e3 / 2**30, 2), "algorithmic_bytes": int(algo),
            "hbm_peak_share": round(algo / (med * 1e-3) / HBM_PEAK, 4), "index_bytes": int(index)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 22)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--host-n", type=int, default=1 << 20)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--no-side-legs", action="store_true", help="the three device legs only")
    a = ap.parse_args()
    side = {} if a.no_side_legs else {"host": host_leg(a.host_n, a.host_threads), "copy_probe": probe_leg(a.n)}
    import torch

    import hysteria_amd
    from hysteria_amd import udpmsg
    if not torch.cuda.is_available():
        raise SystemExit("bench_udpmsg.py needs a GPU: nothing is measured without one")
    dev, n = torch.device("cuda", 0), a.n
    lens = torch.empty(n, dtype=torch.int32, device=dev)
    hysteria_amd.synth_bimodal_lengths(lens, n, 5)
    off = torch.cumsum(lens.to(torch.int64), 0) - lens
    payload = int(off[-1].item() + lens[-1].item())
    data = torch.empty(payload + 16, dtype=torch.uint8, device=dev)
    hysteria_amd.synth_stream(data, payload, 6)
    meta = np.zeros(n, udpmsg.META_DTYPE)
    meta["session_id"] = np.arange(n, dtype=np.uint32)
    meta["packet_id"] = 1 + np.arange(n) % 65535
    meta["max_size"], meta["addr_len"] = 1200, len(ADDR)
    d_meta = torch.from_numpy(meta.view(np.uint8).copy()).to(dev)
    d_addrs = torch.from_numpy(np.frombuffer(ADDR, np.uint8).copy()).to(dev)
    first = torch.empty(n + 1, dtype=torch.int64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    totals = torch.zeros(2, dtype=torch.int64, device=dev)
    ws = torch.empty(udpmsg.frag_workspace_size(n), dtype=torch.uint8, device=dev)
    udpmsg.frag_batch(data, off, lens, d_meta, d_addrs, n, None, 0, None, None, 0, first, status, totals, ws)   # sizing run
    out_bytes, nd = (int(x) for x in totals.cpu())
    out = torch.empty(out_bytes + 16, dtype=torch.uint8, device=dev)
    dgram_off = torch.empty(nd, dtype=torch.int64, device=dev)
    dgram_len = torch.empty(nd, dtype=torch.int32, device=dev)

    def frag():
        udpmsg.frag_batch(data, off, lens, d_meta, d_addrs, n, out, out_bytes, dgram_off, dgram_len, nd, first, status,
                          totals, ws)
    res = {"n": n, "datagrams": nd, "payload_bytes": payload, "datagram_bytes": out_bytes, "max_size": 1200,
           "addr_len": len(ADDR), "steps": a.steps, "warmup": a.warmup, "build_id": hysteria_amd.build_id(),
           "device": torch.cuda.get_device_name(0)}
    res["frag"] = leg(n, payload, payload + out_bytes, n * (8 + 4 + 24) * 3 + n * (8 + 4) + nd * 12,
                      timed(torch, frag, a.steps, a.warmup))
    assert int((status != 0).sum()) == 0 and (int(totals[0]), int(totals[1])) == (out_bytes, nd)

    parsed = torch.empty(nd * 32, dtype=torch.uint8, device=dev)
    res["parse"] = leg(nd, payload, 0, nd * (8 + 4 + 32),
                       timed(torch, lambda: udpmsg.parse_batch(out, dgram_off, dgram_len, nd, parsed), a.steps, a.warmup))
    res["parse"]["note"] = "reads the header bytes only: no algorithmic payload traffic; msgs_per_s counts datagrams"
    assert int((parsed.view(torch.int32)[::8] != 0).sum()) == 0

    frag_idx = torch.arange(nd, dtype=torch.int32, device=dev)
    back = torch.empty(payload + 16, dtype=torch.uint8, device=dev)
    back_len = torch.empty(n, dtype=torch.int32, device=dev)
    back_st = torch.empty(n, dtype=torch.int32, device=dev)
    res["assemble"] = leg(n, payload, 2 * payload, nd * (4 + 8 + 32) + n * (8 + 8 + 4 + 4 + 4),
                          timed(torch, lambda: udpmsg.assemble_batch(out, dgram_off, parsed, nd, frag_idx, first, n, back, off,
                                                                     lens, back_len, back_st), a.steps, a.warmup))
    assert int((back_st != 0).sum()) == 0 and torch.equal(back[:payload], data[:payload])   # the round trip is the identity
    res.update(side)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
