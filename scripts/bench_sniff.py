"""Cost of the server-name stage of the batched QUIC sniffer on one GPU: N client
Initial packets of ~1200 bytes whose CRYPTO data is a well-formed ClientHello
with SNI (64 templates, V1 and V2, one or two CRYPTO frames + PADDING), device
resident.  In one process, interleaved step by step:

  fused   hyobfs_quic_sniff_batch (ReadCryptoPayload, then the SNI kernel)
  plain   hyobfs_quic_read_crypto_payload_batch alone
  sni     hyobfs_tls_client_hello_sni_batch alone, over the assembled payloads

Prints one JSON line: packets/s of fused and plain, the stage's share, and the
stand-alone kernel's ms and achieved bytes/s (payload bytes read + names and
records written) against the HBM peak DESIGN.md section 6 uses (8.0 TB/s).

  python scripts/bench_sniff.py [--n 262144] [--steps 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12


def templates(k=64, seed=12):
    """k client Initials, each with a ClientHello of 250-600 bytes naming its own host."""
    import quic_cases as qc
    import sniff_cases as sc
    from oracle import quic_ref as ref
    rng = np.random.default_rng(seed)
    out = []
    for t in range(k):
        host = (b"host%02d." % t) + b"sub." * int(rng.integers(0, 6)) + b"example.net"
        exts = [(0x0a, b"\x00\x04\x00\x1d\x00\x17"), (0x0b, b"\x01\x00"), (0x23, b""), (0x10, b"\x00\x0c\x02h2\x08http/1.1"),
                (0x0d, bytes(20)), (0x33, rng.integers(0, 256, 38, dtype=np.uint8).tobytes()),
                (0x2b, b"\x02\x03\x04"), (0x2d, b"\x01\x01")]
        at = int(rng.integers(0, len(exts) + 1))
        exts.insert(at, (0, sc.sni_body([(0, host)])))
        exts.append((21, bytes(int(rng.integers(0, 300)))))
        ch = sc.hello(exts, suites=bytes(range(32)))
        if t % 2:
            cut = int(rng.integers(1, len(ch)))
            frames = qc._crypto(cut, ch[cut:]) + b"\x00" * int(rng.integers(0, 40)) + qc._crypto(0, ch[:cut])
        else:
            frames = qc._crypto(0, ch)
        dcid = rng.integers(0, 256, int(rng.integers(8, 21)), dtype=np.uint8).tobytes()
        pad = 1200 - (len(frames) + 30 + len(dcid))
        out.append((ref.client_initial(dcid, b"", ref.V2 if t % 4 > 1 else ref.V1, b"", 2, 4,
                                       frames + b"\x00" * max(pad, 0)), host, len(ch)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    from hysteria_amd import quic, sniff
    dev = torch.device("cuda", 0)
    temps = templates()
    n = args.n
    pick = np.random.default_rng(5).integers(0, len(temps), n)
    lens = np.array([len(temps[i][0]) for i in pick], np.uint32)
    off = np.zeros(n, np.uint64)
    np.cumsum(lens[:-1], out=off[1:])
    src = torch.from_numpy(np.concatenate([np.frombuffer(temps[i][0], np.uint8) for i in pick] +
                                          [np.zeros(64, np.uint8)])).to(dev)
    buf = torch.empty_like(src)
    d_off, d_len = torch.from_numpy(off).to(dev), torch.from_numpy(lens).to(dev)
    cap, stride = 1024, 255
    d_out = torch.empty(n * cap, dtype=torch.uint8, device=dev)
    d_oo = torch.from_numpy(np.arange(n, dtype=np.uint64) * np.uint64(cap)).to(dev)
    d_cap = torch.full((n,), cap, dtype=torch.int32, device=dev)
    d_qres = torch.empty(n * 24, dtype=torch.uint8, device=dev)
    d_names = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    d_sres = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    ws = torch.empty(sniff.quic_sniff_workspace_size(n), dtype=torch.uint8, device=dev)

    def fused():
        sniff.quic_sniff_batch(buf, d_off, d_len, n, d_out, d_oo, d_cap, d_qres, d_names, stride, d_sres, ws)

    def plain():
        quic.read_crypto_payload_batch(buf, d_off, d_len, n, d_out, d_oo, d_cap, d_qres, ws)

    for _ in range(args.warmup):
        for f in (fused, plain):
            buf.copy_(src)   # both calls work in place: restore the protected packets (not timed)
            f()
    torch.cuda.synchronize()
    # the payload lengths the stand-alone kernel reads: out_len of every packet
    qres = np.frombuffer(d_qres.cpu().numpy().tobytes(), quic.RESULT_DTYPE)
    assert (qres["status"] == 0).all(), np.unique(qres["status"])
    d_plen = torch.from_numpy(qres["out_len"].astype(np.uint32)).to(dev)

    def sni():
        sniff.client_hello_sni_batch(d_out, d_oo, d_plen, n, d_names, stride, d_sres)

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = {"fused": [], "plain": [], "sni": []}
    for _ in range(args.steps):
        for name, f in (("fused", fused), ("plain", plain), ("sni", sni)):
            if name != "sni":
                buf.copy_(src)
            ev[0].record()
            f()
            ev[1].record()
            torch.cuda.synchronize()
            ms[name].append(ev[0].elapsed_time(ev[1]))
    sres = np.frombuffer(d_sres.cpu().numpy().tobytes(), sniff.SNIFF_RESULT_DTYPE)
    assert (sres["status"] == 0).all(), np.unique(sres["status"])
    names = d_names.cpu().numpy().reshape(n, stride)
    for i in range(0, n, max(n // 997, 1)):
        assert names[i, :sres["name_len"][i]].tobytes() == temps[pick[i]][1], i
    med = {k: float(np.median(v)) for k, v in ms.items()}
    sni_bytes = int(qres["out_len"].astype(np.uint64).sum() + sres["name_len"].astype(np.uint64).sum() + 16 * n)
    line = {
        "metric": "QUIC sniff (ReadCryptoPayload + ClientHello SNI) packets/s, device resident, ~1200 B client Initials",
        "value": round(n / (med["fused"] / 1e3)), "unit": "packets/s", "n_packets": n, "steps": args.steps,
        "fused_ms": round(med["fused"], 4), "plain_ms": round(med["plain"], 4),
        "plain_packets_per_s": round(n / (med["plain"] / 1e3)),
        "fused_over_plain": round(med["fused"] / med["plain"], 4),
        "fused_ms_min_max": [round(min(ms["fused"]), 4), round(max(ms["fused"]), 4)],
        "plain_ms_min_max": [round(min(ms["plain"]), 4), round(max(ms["plain"]), 4)],
        "sni_kernel": {"ms": round(med["sni"], 4), "ms_min_max": [round(min(ms["sni"]), 4), round(max(ms["sni"]), 4)],
                       "bytes": sni_bytes, "achieved_GBs": round(sni_bytes / (med["sni"] / 1e3) / 1e9, 2),
                       "fraction_of_hbm_peak": round(sni_bytes / (med["sni"] / 1e3) / HBM_PEAK, 5),
                       "mean_hello_bytes": round(float(qres["out_len"].mean()), 1),
                       "messages_per_s": round(n / (med["sni"] / 1e3))},
        "timing": "median of per-step HIP event times, the three legs interleaved in one process",
        "build_id": sniff._slib().hyobfs_build_id().decode()}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
