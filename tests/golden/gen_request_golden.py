#!/usr/bin/env python3
"""Generate tests/golden/request_vectors.json -- fixtures of the request hook
(include/hyobfs_request.h).

"go": the reference's own test tables, transcribed as data
(core/internal/protocol/proxy_test.go:128-330, extras/sniff/sniff_test.go:15-36,
extras/utils/portunion_test.go:9-103).  "lattice": the expected outputs of the
lattice of tests/request_cases.py from the restatement (tests/request_ref.py);
tests/test_request.py holds the restatement to the "go" tables and the library to
both.

Usage:  python tests/golden/gen_request_golden.py          (rewrites the fixture)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import request_cases as rc  # noqa: E402


def hx(s: str) -> str:
    return s.encode("latin-1").hex()


GO = {
    "read_tcp_request": [   # (name, data, want, wantErr)
        {"name": "normal no padding", "data": hx("\x0egoogle.com:443\x00"), "want": "google.com:443", "err": False},
        {"name": "normal with padding", "data": hx("\x0bholy.cc:443\x02gg"), "want": "holy.cc:443", "err": False},
        {"name": "incomplete 1", "data": hx("\x0bhoho"), "want": "", "err": True},
        {"name": "incomplete 2", "data": hx("\x0bholy.cc:443\x05x"), "want": "", "err": True},
    ],
    "write_tcp_request": [   # (name, addr, the prefix of what is written)
        {"name": "normal 1", "addr": "google.com:443", "prefix": hx("\x44\x01\x0egoogle.com:443")},
        {"name": "normal 2", "addr": "client-api.arkoselabs.com:8080", "prefix": hx("\x44\x01\x1eclient-api.arkoselabs.com:8080")},
        {"name": "empty", "addr": "", "prefix": hx("\x44\x01\x00")},
    ],
    "read_tcp_response": [   # (name, data, ok, message, wantErr)
        {"name": "normal ok no padding", "data": hx("\x00\x0bhello world\x00"), "ok": True, "msg": "hello world", "err": False},
        {"name": "normal error with padding", "data": hx("\x01\x06stop!!\x05xxxxx"), "ok": False, "msg": "stop!!", "err": False},
        {"name": "normal ok no message with padding", "data": hx("\x01\x00\x05xxxxx"), "ok": False, "msg": "", "err": False},
        {"name": "incomplete 1", "data": hx("\x00\x0bhoho"), "ok": False, "msg": "", "err": True},
        {"name": "incomplete 2", "data": hx("\x01\x05jesus\x05x"), "ok": False, "msg": "", "err": True},
    ],
    "write_tcp_response": [   # (name, ok, message, the prefix of what is written)
        {"name": "normal ok", "ok": True, "msg": "hello world", "prefix": hx("\x00\x0bhello world")},
        {"name": "normal error", "ok": False, "msg": "stop!!", "prefix": hx("\x01\x06stop!!")},
        {"name": "empty", "ok": True, "msg": "", "prefix": hx("\x00\x00")},
    ],
    "sniffer_check": [   # the sniffer's fields as the test sets them, step by step: (rewrite_domain, tcp, udp, is_udp, addr, want)
        {"rewrite_domain": False, "tcp": None, "udp": None, "is_udp": False, "addr": "1.1.1.1:80", "want": True},
        {"rewrite_domain": False, "tcp": None, "udp": None, "is_udp": False, "addr": "example.com:443", "want": False},
        {"rewrite_domain": True, "tcp": None, "udp": None, "is_udp": False, "addr": "example.com:443", "want": True},
        {"rewrite_domain": True, "tcp": [[80, 80]], "udp": None, "is_udp": False, "addr": "google.com:80", "want": True},
        {"rewrite_domain": True, "tcp": [[80, 80]], "udp": None, "is_udp": False, "addr": "google.com:443", "want": False},
        {"rewrite_domain": True, "tcp": [[80, 80]], "udp": [[443, 443]], "is_udp": True, "addr": "google.com:443", "want": True},
        {"rewrite_domain": True, "tcp": [[80, 80]], "udp": [[443, 443]], "is_udp": True, "addr": "google.com:80", "want": False},
    ],
    "parse_port_union": [   # (name, s, want; null is nil)
        {"name": "empty", "s": "", "want": None},
        {"name": "all 1", "s": "all", "want": [[0, 65535]]},
        {"name": "all 2", "s": "*", "want": [[0, 65535]]},
        {"name": "single port", "s": "1234", "want": [[1234, 1234]]},
        {"name": "multiple ports (unsorted)", "s": "5678,1234,9012", "want": [[1234, 1234], [5678, 5678], [9012, 9012]]},
        {"name": "one range", "s": "1234-1240", "want": [[1234, 1240]]},
        {"name": "one range (reversed)", "s": "1240-1234", "want": [[1234, 1240]]},
        {"name": "multiple ports and ranges (reversed, unsorted, overlapping)", "s": "5678,1200-1236,9100-9012,1234-1240",
         "want": [[1200, 1240], [5678, 5678], [9012, 9100]]},
        {"name": "multiple ports and ranges with 65535 (reversed, unsorted, overlapping)",
         "s": "5678,1200-1236,65531-65535,65532-65534,9100-9012,1234-1240",
         "want": [[1200, 1240], [5678, 5678], [9012, 9100], [65531, 65535]]},
        {"name": "multiple ports and ranges with 65535 (reversed, unsorted, overlapping) 2",
         "s": "5678,1200-1236,65532-65535,65531-65534,9100-9012,1234-1240",
         "want": [[1200, 1240], [5678, 5678], [9012, 9100], [65531, 65535]]},
        {"name": "invalid 1", "s": "1234-", "want": None},
        {"name": "invalid 2", "s": "1234-ggez", "want": None},
        {"name": "invalid 3", "s": "233,", "want": None},
        {"name": "invalid 4", "s": "1234-1240-1250", "want": None},
        {"name": "invalid 5", "s": "-,,", "want": None},
        {"name": "invalid 6", "s": "http", "want": None},
    ],
}


def main() -> None:
    doc = {"go": GO, "lattice": rc.golden_lattice()}
    path = os.path.join(HERE, "request_vectors.json")
    with open(path, "w") as f:   # one vector per line
        f.write("{\n")
        for i, (top, tables) in enumerate(sorted(doc.items())):
            f.write(f' "{top}": {{\n')
            for j, (name, rows) in enumerate(sorted(tables.items())):
                body = ",\n".join("   " + json.dumps(r, sort_keys=True) for r in rows)
                f.write(f'  "{name}": [\n{body}\n  ]' + ("," if j + 1 < len(tables) else "") + "\n")
            f.write(" }" + ("," if i + 1 < len(doc) else "") + "\n")
        f.write("}\n")
    json.load(open(path))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
