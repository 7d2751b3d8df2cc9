"""Cost of large DOMAIN_SETs with and without the hashed index (include/hyobfs_acl.h,
"THE INDEX"; hysteria_amd/csrc/acl.hip) on one GPU.  One process; the same rules
compiled linear and indexed, the two interleaved step by step; every timing the
median of per-step HIP event times after warm-up.  Both must give the same records.

  sets4096   bench_acl.py's 64-rule set: two DOMAIN_SETs of 4096 root values and a
             CIDR_SET of 8192 (8254 entries linear, 64 indexed)
  geosite    direct(set of 65,029) proxy(set of 19,300) reject(set of 65,792)
             rest(all): the sizes of the reference geosite.dat's cn (64,590 root, 402
             full, 37 regex), geolocation-!cn (18,754 / 440 / 106) and category-ads-all
             (all root).  The values are synthetic from a seed, 99 % of two labels as
             in cn; the regexes are those of tests/golden/geosite_regex.json

Name mixes per leg: miss (no set holds the name), mixed (a third each in the first
set, in the last set, in none), and misses of 1, 3 and 8 labels.

Prints one JSON line and writes it to profiles/acl/bench_acl_index.json (--out).

  python scripts/bench_acl_index.py [--n 262144] [--steps 10] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

TEMPLATES = 4096


def geosite_rules(seed=20):
    """The four rules of the geosite-scale set as acl.Rule objects."""
    from hysteria_amd import acl
    with open(os.path.join(ROOT, "tests", "golden", "geosite_regex.json"), encoding="utf-8") as f:
        fx = json.load(f)
    rnd = random.Random(seed)

    def values(count, tag, tld):
        out = []
        for k in range(count):
            word = "".join(rnd.choice("abcdefghijklmnopqrstuvwxyz0123456789") for _ in range(rnd.randrange(3, 12)))
            out.append("%s%s%d.%s%s" % (word, tag, k, "sub." if k % 100 == 99 else "", tld))   # 1 % of three labels
        return out
    rules = []
    for tag, tld, roots, fulls, regex_list, outbound in (("a", "cn", 64590, 402, "cn", 1), ("b", "com", 18754, 440, "geolocation-!cn", 2),
                                                          ("c", "net", 65792, 0, None, 3)):
        ents = [("root", v) for v in values(roots, tag, tld)] + [("full", v) for v in values(fulls, tag + "f", tld)]
        if regex_list:
            ents += [("regex", v) for n, v, a in fx["entries"] if n == regex_list]
        r = acl.Rule(acl.KIND_DOMAIN_SET, entries=ents)
        r.outbound = outbound
        rules.append(r)
    rest = acl.Rule(acl.KIND_ALL)
    rest.outbound = 4
    rules.append(rest)
    for i, r in enumerate(rules):
        r.line_num = i + 1
    return rules


def mixes(first, last):
    """Template names per mix; `first` / `last`: the root values of the first and the last set."""
    def miss(k, labels=3):
        return ".".join(["l%d" % j for j in range(labels - 3)] + ["host%04d" % k, "sub%d" % (k % 5), "example"][:min(labels, 3)])
    out = {"miss": [miss(k) for k in range(TEMPLATES)],
           "mixed": [("h%d.%s" % (k, first[(7 * k) % len(first)]), "h%d.%s" % (k, last[(7 * k) % len(last)]), miss(k))[k % 3]
                     for k in range(TEMPLATES)]}
    for labels in (1, 3, 8):
        out["miss_%d_labels" % labels] = [miss(k, labels) for k in range(TEMPLATES)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "acl", "bench_acl_index.json"))
    args = ap.parse_args()
    import torch
    from bench_acl import rule_set
    from hysteria_amd import acl, sniff
    if not torch.cuda.is_available():
        raise SystemExit("bench_acl_index.py needs a GPU: there is no CPU fallback")
    dev = torch.device("cuda", 0)
    n = args.n
    rng = np.random.default_rng(7)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    d_res = {k: torch.empty(n * 16, dtype=torch.uint8, device=dev) for k in ("linear", "indexed")}
    d_proto = torch.full((n,), acl.PROTO_TCP, dtype=torch.uint8, device=dev)
    d_port = torch.full((n,), 443, dtype=torch.int16, device=dev)

    def leg(sets, temps):
        """Median / min / max ms of linear and indexed over n names drawn from temps, interleaved."""
        pick = rng.integers(0, len(temps), n)
        lens = np.array([len(t) for t in temps], np.uint32)[pick]
        off = np.zeros(n, np.uint64)
        np.cumsum(lens[:-1], out=off[1:])
        blob = np.frombuffer("".join(temps[i] for i in pick).encode() + bytes(16), np.uint8).copy()
        d_names, d_off, d_len = torch.from_numpy(blob).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(lens).to(dev)
        ms = {k: [] for k in sets}
        for step in range(args.warmup + args.steps):
            for k, rs in sets.items():
                ev[0].record()
                rs.match_batch(d_names, d_off, d_len, None, None, None, d_proto, d_port, n, d_res[k])
                ev[1].record()
                torch.cuda.synchronize()
                if step >= args.warmup:
                    ms[k].append(ev[0].elapsed_time(ev[1]))
        res = {k: np.frombuffer(d_res[k].cpu().numpy().tobytes(), acl.ACL_RESULT_DTYPE) for k in sets}
        assert (res["linear"]["status"] == 0).all() and res["linear"].tobytes() == res["indexed"].tobytes()
        out = {k: {"ms": round(float(np.median(v)), 4), "ms_min_max": [round(min(v), 4), round(max(v), 4)],
                   "names_per_s": round(n / (float(np.median(v)) / 1e3))} for k, v in ms.items()}
        out["speedup"] = round(out["linear"]["ms"] / out["indexed"]["ms"], 2)
        out["matched_fraction"] = round(float((res["linear"]["rule"] >= 0).mean()), 4)
        return out

    line = {"metric": "ACL match_batch ms per batch, large DOMAIN_SETs, linear walk against the hashed index",
            "unit": "ms", "n_names": n, "steps": args.steps, "legs": {}}
    small = rule_set(64, True)
    big = geosite_rules()
    for label, rules, first, last in (("sets4096", small.rules, small.rules[20].entries, small.rules[40].entries),
                                      ("geosite", big, big[0].entries[:64590], big[2].entries)):
        sets = {"linear": acl.RuleSet(rules), "indexed": acl.RuleSet(rules, device_index=True)}
        hs = {k: rs.device_set(0) for k, rs in sets.items()}
        rec = {"entries": {k: acl.ruleset_entries(h) for k, h in hs.items()},
               "index": {str(r): acl.ruleset_index_info(hs["indexed"], r)._asdict() for r in range(len(rules))
                         if acl.ruleset_index_info(hs["indexed"], r).slots}}
        for mix, temps in mixes([e[1] for e in first], [e[1] for e in last]).items():
            rec[mix] = leg(sets, temps)
        line["legs"][label] = rec
        for rs in sets.values():
            rs.close()
    line["value"] = line["legs"]["geosite"]["mixed"]["indexed"]["ms"]
    line["timing"] = "median of per-step HIP event times after warm-up; linear and indexed interleaved in one process"
    line["build_id"] = sniff._slib().hyobfs_build_id().decode()
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
