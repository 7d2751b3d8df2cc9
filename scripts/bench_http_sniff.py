"""Cost of the sniffer's HTTP branch and TCP dispatch on one GPU, device resident.
In one process, interleaved step by step:

  http     hyobfs_http_request_host_batch over N requests of a seeded realistic
           mix (256 templates, about 150-600 bytes of headers, a third with a body)
  tcp      hyobfs_tcp_sniff_batch over the same requests
  http2k   hyobfs_http_request_host_batch over N / 4 requests with 2 KiB of headers
  tls      hyobfs_tls_record_sni_batch over N TLS records holding ClientHellos of
           250-600 bytes (the recipe of scripts/bench_sniff.py): the sibling figure

Prints one JSON line: per leg the median ms of per-step HIP event times, its
spread, streams/s and the achieved GB/s over the bytes the parse must read (the
header block up to its blank line, or the record) plus the names and records
written.

  python scripts/bench_http_sniff.py [--n 1048576] [--steps 20] [--warmup 3] [--out FILE] [--lib PATH]

--lib loads another build of libhyobfs.so (an A/B variant) instead of the package's.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

AGENTS = [b"Mozilla/5.0 (X11; Linux x86_64) AppleWebKit/537.36 (KHTML, like Gecko) Chrome/126.0.0.0 Safari/537.36",
          b"Mozilla/5.0 (Macintosh; Intel Mac OS X 14_5) AppleWebKit/605.1.15 (KHTML, like Gecko) Version/17.5 Safari/605.1.15",
          b"curl/8.5.0", b"Go-http-client/1.1", b"okhttp/4.12.0", b"python-requests/2.32.3",
          b"Mozilla/5.0 (Windows NT 10.0; Win64; x64; rv:127.0) Gecko/20100101 Firefox/127.0"]


def _token(rng, n):
    return bytes(rng.choice(np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789", np.uint8), n))


def request_templates(k=256, seed=21, target=None):
    """k valid requests, each naming its own host: (bytes, host, header bytes).
    target: pad the header block with cookies to about this many bytes."""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(k):
        host = (b"h%03d." % t) + b"cdn." * int(rng.integers(0, 4)) + b"example.net"
        port = b":8080" if t % 5 == 0 else b""
        post = t % 3 == 0
        path = b"/" + b"/".join(_token(rng, int(rng.integers(3, 12))) for _ in range(int(rng.integers(1, 5))))
        if t % 4 == 1:
            path += b"?q=" + _token(rng, int(rng.integers(4, 30))) + b"%20x"
        head = [b"User-Agent: " + AGENTS[t % len(AGENTS)], b"Accept: text/html,application/xhtml+xml;q=0.9,*/*;q=0.8",
                b"Accept-Encoding: gzip, deflate", b"Connection: keep-alive"]
        if t % 2:
            head.append(b"Accept-Language: en-US,en;q=0.5")
        if t % 3 == 1:
            head.append(b"Referer: http://" + host + b"/" + _token(rng, int(rng.integers(5, 40))))
        if t % 4 < 2:
            head.append(b"Cookie: sid=" + _token(rng, int(rng.integers(16, 200))))
        body = b""
        if post:
            body = _token(rng, int(rng.integers(10, 120)))
            head += [b"Content-Type: application/x-www-form-urlencoded", b"Content-Length: %d" % len(body)]
        head = [head[i] for i in rng.permutation(len(head))]
        head.insert(int(rng.integers(0, len(head) + 1)), b"Host: " + host + port)
        line = (b"POST " if post else b"GET ") + path + b" HTTP/1.1"
        block = line + b"\r\n" + b"".join(h + b"\r\n" for h in head) + b"\r\n"
        while target and len(block) < target:   # cookies of 60-200 bytes up to the target
            head.insert(int(rng.integers(0, len(head) + 1)),
                        b"X-" + _token(rng, 6) + b": " + _token(rng, min(int(rng.integers(60, 200)), max(target - len(block) - 12, 1))))
            block = line + b"\r\n" + b"".join(h + b"\r\n" for h in head) + b"\r\n"
        out.append((block + body, host, len(block)))
    return out


def record_templates(k=64, seed=12):
    """k TLS records, each a ClientHello of 250-600 bytes naming its own host
    (the hello recipe of scripts/bench_sniff.py)."""
    import sniff_cases as sc
    rng = np.random.default_rng(seed)
    out = []
    for t in range(k):
        host = (b"host%02d." % t) + b"sub." * int(rng.integers(0, 6)) + b"example.net"
        exts = [(0x0a, b"\x00\x04\x00\x1d\x00\x17"), (0x0b, b"\x01\x00"), (0x23, b""), (0x10, b"\x00\x0c\x02h2\x08http/1.1"),
                (0x0d, bytes(20)), (0x33, rng.integers(0, 256, 38, dtype=np.uint8).tobytes()),
                (0x2b, b"\x02\x03\x04"), (0x2d, b"\x01\x01")]
        exts.insert(int(rng.integers(0, len(exts) + 1)), (0, sc.sni_body([(0, host)])))
        exts.append((21, bytes(int(rng.integers(0, 300)))))
        rec = sc.as_record(sc.hello(exts, suites=bytes(range(32))))
        out.append((rec, host, len(rec)))
    return out


class Leg:
    def __init__(self, dev, temps, n, seed, stride=255):
        import torch
        self.temps, self.n, self.stride = temps, n, stride
        self.pick = np.random.default_rng(seed).integers(0, len(temps), n)
        lens = np.array([len(t[0]) for t in temps], np.uint32)[self.pick]
        off = np.zeros(n, np.uint64)
        np.cumsum(lens[:-1], out=off[1:])
        width = max(len(t[0]) for t in temps)
        rows = np.zeros((len(temps), width), np.uint8)
        for i, t in enumerate(temps):
            rows[i, :len(t[0])] = np.frombuffer(t[0], np.uint8)
        flat = np.empty(int(lens.sum()) + 64, np.uint8)
        flat[-64:] = 0
        mask = np.arange(width)[None, :] < np.array([len(t[0]) for t in temps])[:, None]
        step = 1 << 16   # gather in slices: the mask of a million rows at once would be large
        at = 0
        for s in range(0, n, step):
            p = self.pick[s:s + step]
            part = rows[p][mask[p]]
            flat[at:at + len(part)] = part
            at += len(part)
        self.buf = torch.from_numpy(flat).to(dev)
        self.off, self.len = torch.from_numpy(off).to(dev), torch.from_numpy(lens).to(dev)
        self.names = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
        self.res = torch.empty(n * 16, dtype=torch.uint8, device=dev)
        self.read_bytes = int(np.array([t[2] for t in temps], np.uint64)[self.pick].sum())

    def run(self, call):
        call(self.buf, self.off, self.len, self.n, self.names, self.stride, self.res)

    def verify(self, sniff):
        res = np.frombuffer(self.res.cpu().numpy().tobytes(), sniff.SNIFF_RESULT_DTYPE)
        assert (res["status"] == 0).all(), np.unique(res["status"])
        names = self.names.cpu().numpy().reshape(self.n, self.stride)
        for i in range(0, self.n, max(self.n // 997, 1)):
            assert names[i, :res["name_len"][i]].tobytes() == self.temps[self.pick[i]][1], i
        return int(res["name_len"].astype(np.uint64).sum()) + 16 * self.n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--lib", help="a libhyobfs.so to load instead of the package's")
    args = ap.parse_args()
    if args.lib:
        os.environ["HYOBFS_LIB"] = os.path.abspath(args.lib)
    import torch
    from hysteria_amd import _lib, sniff
    if args.lib:
        assert os.path.samefile(_lib.load()._name, args.lib), "the package loaded another library"
    dev = torch.device("cuda", 0)
    mix = Leg(dev, request_templates(), args.n, 5)
    big = Leg(dev, request_templates(64, 22, target=2048), max(args.n // 4, 1), 6)
    tls = Leg(dev, record_templates(), args.n, 7)
    legs = {"http": (mix, sniff.http_request_host_batch), "tcp": (mix, sniff.tcp_sniff_batch),
            "http2k": (big, sniff.http_request_host_batch), "tls": (tls, sniff.tls_record_sni_batch)}
    for _ in range(args.warmup):
        for leg, call in legs.values():
            leg.run(call)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = {k: [] for k in legs}
    for _ in range(args.steps):
        for name, (leg, call) in legs.items():
            ev[0].record()
            leg.run(call)
            ev[1].record()
            torch.cuda.synchronize()
            ms[name].append(ev[0].elapsed_time(ev[1]))
    line = {"metric": "HTTP sniff (request host of a seeded realistic mix) requests/s, device resident",
            "unit": "requests/s", "steps": args.steps,
            "timing": "median of per-step HIP event times, the four legs interleaved in one process",
            "build_id": sniff._slib().hyobfs_build_id().decode(), "lib": args.lib or "package"}
    for name, (leg, call) in legs.items():
        leg.run(call)
        written = leg.verify(sniff)
        med = float(np.median(ms[name]))
        line[name] = {"n": leg.n, "ms": round(med, 4), "ms_min_max": [round(min(ms[name]), 4), round(max(ms[name]), 4)],
                      "per_s": round(leg.n / (med / 1e3)), "mean_read_bytes": round(leg.read_bytes / leg.n, 1),
                      "mean_stream_bytes": round(float(leg.len.float().mean()), 1),
                      "read_GBs": round(leg.read_bytes / (med / 1e3) / 1e9, 2),
                      "read_plus_written_GBs": round((leg.read_bytes + written) / (med / 1e3) / 1e9, 2)}
    line["value"] = line["http"]["per_s"]
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
