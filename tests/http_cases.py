"""HTTP request cases for the sniffer's HTTP branch and its TCP dispatch
(hysteria_amd/csrc/sniff_http.h, sniff.hip), shared by the CPU tier
(tests/test_http_sniff.py, through tests/emu/http_main.cpp) and the GPU tier
(tests/test_gpu_http_sniff.py).  Built from the rules alone; expected results
come from tests/http_ref.py.
"""
import functools

import numpy as np

import http_ref
import sniff_cases as sc

SENTINEL = sc.SENTINEL
NAME_STRIDE = sc.NAME_STRIDE
MAX = http_ref.MAX_HEADER_BYTES
GRID_CAP_MSGS = sc.GRID_CAP_MSGS   # sniff.hip: kGridCap workgroups of kWaves streams


def req(line=b"GET / HTTP/1.1", headers=(b"Host: example.com",), eol=b"\r\n", body=b""):
    return line + eol + b"".join(h + eol for h in headers) + eol + body


@functools.lru_cache(maxsize=None)
def lattice_cases():
    """(name, first bytes of a stream): an accepting and a rejecting case per clause of H0-H7."""
    h = b"Host: example.com"
    c = [
        # H0
        ("valid", req()),
        ("valid_post_body", req(b"POST /hello HTTP/1.1", (h, b"Content-Length: 5"), body=b"hello")),
        ("h0_len_0", b""), ("h0_len_2", b"GE"), ("h0_len_3", b"GET"), ("h0_digit_third", b"GE1 / HTTP/1.1\r\n\r\n"),
        ("h0_at_first", b"@ET / HTTP/1.1\r\n\r\n"), ("h0_bracket_second", b"G[T / HTTP/1.1\r\n\r\n"),
        ("h0_lower", req(b"get / HTTP/1.1")), ("h0_edges_AZaz", req(b"AZaz / HTTP/1.1")),
        ("h0_brace_third", b"GE{ / HTTP/1.1\r\n\r\n"), ("h0_backtick", b"`ET / HTTP/1.1\r\n\r\n"),
        # H1
        ("h1_no_space", req(b"GET/HTTP/1.1")), ("h1_one_space", req(b"GET /HTTP/1.1")),
        ("h1_three_spaces", req(b"GET / x HTTP/1.1")), ("h1_tab_not_space", req(b"GET\t/\tHTTP/1.1")),
        # H2
        ("h2_method_tchars", req(b"GET!#$%&'*+-.^_`|~09 / HTTP/1.1")), ("h2_method_paren", req(b"GET( / HTTP/1.1")),
        ("h2_method_colon", req(b"GET: / HTTP/1.1")), ("h2_method_0x80", req(b"GET\x80 / HTTP/1.1")),
        ("h2_method_slash", req(b"GET/ / HTTP/1.1")),
        # H3
        ("h3_http_1_0", req(b"GET / HTTP/1.0")), ("h3_http_9_9", req(b"GET / HTTP/9.9")),
        ("h3_http_1_10", req(b"GET / HTTP/1.10")), ("h3_http_11", req(b"GET / HTTP/11")),
        ("h3_lower", req(b"GET / http/1.1")), ("h3_no_dot", req(b"GET / HTTP/1x1")), ("h3_alpha_minor", req(b"GET / HTTP/1.a")),
        ("h3_empty", req(b"GET / ")), ("h3_trailing_space", req(b"GET / HTTP/1.1 ")), ("h3_short", req(b"GET / HTTP/1.")),
        # H4
        ("h4_star", req(b"OPTIONS * HTTP/1.1")), ("h4_star_x", req(b"OPTIONS *x HTTP/1.1")),
        ("h4_empty_uri", req(b"GET  HTTP/1.1")), ("h4_double_slash", req(b"GET //a/b HTTP/1.1")),
        ("h4_pct_ok", req(b"GET /a%2Fb%c3%A9 HTTP/1.1")), ("h4_pct_at_end", req(b"GET /a% HTTP/1.1")),
        ("h4_pct_one_digit_at_end", req(b"GET /a%4 HTTP/1.1")), ("h4_pct_zz_path", req(b"GET /a%zz HTTP/1.1")),
        ("h4_pct_zz_query", req(b"GET /a?b=%zz HTTP/1.1")), ("h4_pct_before_query", req(b"GET /a%?b HTTP/1.1")),
        ("h4_pct_g_second", req(b"GET /%4g HTTP/1.1")), ("h4_pct_in_second_query", req(b"GET /a?b?%zz HTTP/1.1")),
        ("h4_ctl", req(b"GET /a\x01b HTTP/1.1")), ("h4_del", req(b"GET /a\x7fb HTTP/1.1")),
        ("h4_cr_in_uri", req(b"GET /a\rb HTTP/1.1")), ("h4_tab_in_uri", req(b"GET /a\tb HTTP/1.1")),
        ("h4_0x80", req(b"GET /a\x80\xffb HTTP/1.1")), ("h4_ctl_in_query", req(b"GET /a?\x1f HTTP/1.1")),
        ("h4_absolute", req(b"GET http://example.org/x HTTP/1.1")), ("h4_connect", req(b"CONNECT a:1 HTTP/1.1", (b"Host: a:1",))),
        ("h4_absolute_ctl", req(b"GET http://e/\x01 HTTP/1.1")), ("h4_absolute_bad_proto", req(b"GET http://e/ HTTP/11")),
        ("h4_question_first", req(b"GET ?a HTTP/1.1")),
        # H5
        ("h5_first_line_space", req(headers=(b" Host: example.com",))), ("h5_first_line_tab", req(headers=(b"\tx: y", h))),
        ("h5_folded", req(headers=(h, b" folded"))), ("h5_folded_tab", req(headers=(b"A: b", b"\tc", h))),
        ("h5_folded_only_spaces", req(headers=(h, b"   "))), ("h5_folded_then_bad", req(headers=(h, b" x", b"nocolon"))),
        ("h5_bad_then_folded", req(headers=(h, b"nocolon", b" x"))),
        ("h5_no_colon", req(headers=(h, b"nocolon"))), ("h5_no_colon_first", req(headers=(b"Host example.com",))),
        ("h5_key_space", req(headers=(b"Host : example.com",))), ("h5_key_space_inside", req(headers=(b"Ho st: x", h))),
        ("h5_key_tab", req(headers=(b"Host\t: example.com",))), ("h5_key_paren", req(headers=(h, b"X(y): z"))),
        ("h5_key_0x80", req(headers=(h, b"X\x80: z"))), ("h5_key_tchars", req(headers=(b"!#$%&'*+-.^_`|~09aZ: v", h))),
        ("h5_empty_key_good", req(headers=(b": v", h))), ("h5_empty_key_bad", req(headers=(b": v\x01", h))),
        ("h5_value_bare_cr", req(headers=(b"A: b\rc", h))), ("h5_value_nul", req(headers=(b"A: b\x00c", h))),
        ("h5_value_0x80", req(headers=(b"A: b\x80\xffc", h))), ("h5_value_del", req(headers=(b"A: b\x7fc", h))),
        ("h5_value_tab", req(headers=(b"A: b\tc", h))), ("h5_value_colons", req(headers=(b"A: b:c:d", h))),
        ("h5_value_0x1f", req(headers=(b"A: \x1f", h))), ("h5_trailing_ws", req(headers=(b"Host: example.com \t ",))),
        ("h5_leading_ws", req(headers=(b"Host: \t  example.com",))), ("h5_no_ws", req(headers=(b"Host:example.com",))),
        ("h5_double_cr", req(headers=(h + b"\r",))), ("h5_cr_cr_lf_blank", b"GET / HTTP/1.1\r\n" + h + b"\r\n\r\r\n"),
        ("h5_lf_only", req(eol=b"\n")), ("h5_lf_only_post", req(b"POST /p HTTP/1.0", (b"A: b", h, b"C: d"), eol=b"\n")),
        ("h5_mixed_eol", b"GET / HTTP/1.1\n" + h + b"\r\n\n"), ("h5_cr_in_key", req(headers=(b"Ho\rst: x",))),
        ("h5_no_headers", b"GET / HTTP/1.1\r\n\r\n"), ("h5_bad_after_block", req(body=b"nocolon\r\n\x00\r\n")),
        # H6
        ("h6_host_case", req(headers=(b"hOsT: example.com",))), ("h6_two_hosts", req(headers=(h, b"host: other"))),
        ("h6_two_hosts_te", req(headers=(h, b"Transfer-Encoding: chunked", h))),
        ("h6_host_empty", req(headers=(b"Host:",))), ("h6_host_only_ws", req(headers=(b"Host:  \t ",))),
        ("h6_no_host", req(headers=(b"User-Agent: x",))), ("h6_hosts_not", req(headers=(b"Hosts: a", b"Hos: b", b"Xost: c"))),
        ("h6_te", req(headers=(h, b"transfer-ENCODING: chunked"))), ("h6_te_17_other", req(headers=(h, b"Transfer-Encodinx: q"))),
        ("h6_trailer", req(headers=(h, b"Trailer: x"))), ("h6_7_other", req(headers=(h, b"Referer: x", b"Upgrade: y"))),
        ("h6_two_cl", req(headers=(h, b"Content-Length: 1", b"content-length: 1"))),
        ("h6_cl_1x", req(headers=(h, b"Content-Length: 1x"))), ("h6_cl_18", req(headers=(h, b"Content-Length: " + b"9" * 18))),
        ("h6_cl_19", req(headers=(h, b"Content-Length: " + b"1" * 19))), ("h6_cl_empty", req(headers=(h, b"Content-Length:"))),
        ("h6_cl_ws", req(headers=(h, b"Content-Length: \t 27 \t"))), ("h6_cl_plus", req(headers=(h, b"Content-Length: +1"))),
        ("h6_cl_inner_space", req(headers=(h, b"Content-Length: 1 2"))), ("h6_14_other", req(headers=(h, b"Accept-Charset: 1x"))),
        ("h6_cl_bad_need_more", req(headers=(h, b"Content-Length: 1x"))[:-2]),
        ("h6_two_hosts_need_more", req(headers=(h, h))[:-1]),
        # H7
        ("h7_port", req(headers=(b"Host: a:1",))), ("h7_v6_port", req(headers=(b"Host: [::1]:80",))),
        ("h7_v6_no_port", req(headers=(b"Host: [::1]",))), ("h7_colons", req(headers=(b"Host: a:b:c",))),
        ("h7_after_bracket", req(headers=(b"Host: [a]b:1",))), ("h7_stray_rb", req(headers=(b"Host: a]:1",))),
        ("h7_empty_host", req(headers=(b"Host: :80",))), ("h7_empty_brackets", req(headers=(b"Host: []:80",))),
        ("h7_empty_port", req(headers=(b"Host: a:",))), ("h7_stray_lb", req(headers=(b"Host: a[b:1",))),
        ("h7_no_rb", req(headers=(b"Host: [::1:80",))), ("h7_two_rb", req(headers=(b"Host: [a]]:1",))),
        ("h7_lb_inside", req(headers=(b"Host: [[a]:1",))), ("h7_v6_colons_after", req(headers=(b"Host: [::1]:4:3",))),
        ("h7_rb_in_port", req(headers=(b"Host: [a]:1]",))), ("h7_dot_end", req(headers=(b"Host: example.com.:80",))),
        ("h7_ip", req(headers=(b"Host: 10.0.0.1:8080",))), ("h7_space_inside", req(headers=(b"Host: a b:1",))),
        ("h7_0x80", req(headers=(b"Host: \xc3\xa9.example:1",))), ("h7_only_colon", req(headers=(b"Host: :",))),
        ("h7_name_255", req(headers=(b"Host: " + b"a" * 255 + b":1",))), ("h7_name_256", req(headers=(b"Host: " + b"b" * 256,))),
        ("h7_value_300_colons", req(headers=(b"Host: " + b"c:" * 150,))),
        ("h7_v6_long", req(headers=(b"Host: [" + b"1:" * 70 + b":1]:443",))),
    ]
    assert len({n for n, _ in c}) == len(c)
    return tuple(c)


STRIDE_CASES = ("valid", "h7_port", "h7_v6_port", "h6_no_host", "h7_colons")   # names of 11, 1, 3, 0 and 5 bytes


def _lf_at(k):
    """A valid request whose request line's LF is byte k."""
    r = req(b"GET /" + b"a" * (k - 15) + b" HTTP/1.1")
    assert r[k] == 10
    return r


def _host_at(k, filler="line", eol=b"\r\n", host=b"Host: example.com:8080"):
    """A valid request whose Host line starts at byte k (>= 21), behind one long
    header line or behind many short ones."""
    if filler == "line":
        pad = [b"P: " + b"a" * (k - 21)] if eol == b"\r\n" else [b"P: " + b"a" * (k - 19)]
    else:
        n, rest = divmod(k - 16, 8)
        pad = [b"Ab: cd"] * (n - 1) + [b"Ab: cd" + b"e" * rest]
        assert eol == b"\r\n" and n >= 1
    r = req(headers=(*pad, host, b"Accept: */*"), eol=eol)
    assert r[k:k + 5] == b"Host:", (k, r[k:k + 5])
    return r


def _big(total, terminated):
    """A request of `total` bytes: a valid header block (its final LF is the last
    byte) or one that lacks its blank line."""
    head = b"GET / HTTP/1.1\r\nHost: big.example\r\n"
    tail = b"\r\n\r\n" if terminated else b"\r\n"
    lines, left = [], total - len(head) - len(tail) - 3
    while left > 4000:   # long lines and short ones
        lines.append(b"X: " + b"v" * 2997 + b"\r\n" + b"Y: z\r\n" * 166)
        left -= 3002 + 6 * 166
    r = head + b"".join(lines) + b"P: " + b"w" * left + tail
    assert len(r) == total
    return r


@functools.lru_cache(maxsize=None)
def window_cases():
    """The smallest shapes at which the scan can go wrong: line ends, CR LF
    pairs, the colon, the key and the value at the edges of a 64-byte step and
    of the 1024 bytes staged at a time, and the 256 KiB limit."""
    c = [(f"win_reqline_lf_{k}", _lf_at(k)) for k in (62, 63, 64, 65, 127, 128, 1023, 1024)]
    c += [(f"win_reqline_lf_only_{k}", req(b"GET /" + b"a" * (k - 14) + b" HTTP/1.1", eol=b"\n")) for k in (63, 64)]
    c += [(f"win_reqline_pct_{k}_{t.decode()}", req(b"GET /" + b"a" * (k - 5) + b"%4" + t + b" HTTP/1.1"))
          for k in (61, 62, 63, 64) for t in (b"1", b"g")]      # the '%' is byte k
    c += [(f"win_reqline_space_{k}", req(b"G" * k + b" /x HTTP/1.1")) for k in (63, 64, 65)]
    for k in list(range(50, 68)) + list(range(116, 132)) + list(range(1010, 1028)):
        c.append((f"win_host_at_{k}", _host_at(k)))
    for k in (60, 62, 63, 64, 1022, 1023, 1024, 1025):
        c.append((f"win_host_at_{k}_lf_only", _host_at(k, eol=b"\n")))
        c.append((f"win_host_at_{k}_short_lines", _host_at(k, "short")))
    # the block's final CR LF CR LF at every offset from a step's edge
    for k in range(40, 48):
        r = _host_at(k)
        c.append((f"win_end_{len(r) - 1}", r))
    for k in range(990, 998):
        r = _host_at(k)
        c.append((f"win_end_{len(r) - 1}", r))
    # a CR as the last byte of a step that is not followed by LF
    r = req(headers=(b"P: " + b"a" * 42 + b"\rb", b"Host: x"))
    assert r[63] == 13
    c.append(("win_bare_cr_63", r))
    r = req(headers=(b"P" * 47 + b"\rb: c", b"Host: x"))
    assert r[63] == 13
    c.append(("win_bare_cr_63_in_key", r))
    r = req(headers=(b"P: " + b"a" * 43, b"Host: x"))
    assert r[62:64] == b"\r\n"
    c += [("win_line_ends_63", r), ("win_line_ends_63_folded", r[:64] + b" " + r[64:])]
    # a long Host value: the split runs over several steps
    c.append(("win_host_value_200", req(headers=(b"Host: " + b"h" * 200 + b":8080",))))
    c.append(("win_host_value_v6_200", req(headers=(b"Host: [" + b"1:" * 100 + b"]:8080",))))
    c.append(("win_host_ws_100", req(headers=(b"Host:" + b" " * 100 + b"padded.example:1" + b"\t" * 100,))))
    c.append(("win_cl_ws_100", req(headers=(b"Host: x", b"Content-Length:" + b" " * 100 + b"12" + b" " * 70))))
    full = req(headers=(b"Host: example.com", b"Accept: */*"))
    c += [("win_final_lf_last", full), ("win_one_short", full[:-1]), ("win_two_short", full[:-2]),
          ("win_body_follows", full + b"\x00\x01binary\r\n"), ("win_reqline_only", b"GET / HTTP/1.1\r\n"),
          ("win_reqline_incomplete", b"GET / HTTP/1.1\r"), ("win_bad_line_incomplete", full[:-4] + b"\r\nnocolon\r")]
    c += [("win_big_final_lf_262143", _big(MAX, True)),
          ("win_big_final_lf_262144", _big(MAX + 1, True)),
          ("win_big_no_end_262143", _big(MAX - 1, False)),
          ("win_big_no_end_262144", _big(MAX, False)),
          ("win_big_bad_line_past_limit", _big(MAX, False) + b"nocolon\r\n\r\n")]
    assert len({n for n, _ in c}) == len(c), [n for n, _ in c]
    return tuple(c)


def small_window_cases():
    return tuple(x for x in window_cases() if len(x[1]) < 4096)


def big_window_cases():
    return tuple(x for x in window_cases() if len(x[1]) >= 4096)


FUZZ_SEED = 11
_FUZZ_BYTES = b" \t:\r\n%[]/?x0(\x00\x7f\x80"


@functools.lru_cache(maxsize=None)
def fuzz_cases(seed=FUZZ_SEED, count=512):
    """`count` byte-level mutations (flip, insert, delete, truncate) of valid
    requests.  Half of the positions are drawn from the places where the rules
    look (line starts, the request line's fields, colons, value starts)."""
    rng = np.random.default_rng(seed)
    bases = [
        req(b"GET /index.html?q=%41 HTTP/1.1", (b"Host: fuzz.example.net:8080", b"User-Agent: curl/8.5.0", b"Accept: */*")),
        req(b"POST /api/v1/items HTTP/1.1", (b"Host: api.example.org", b"Content-Type: application/json",
                                              b"Content-Length: 27", b"Connection: keep-alive"), body=b"x" * 27),
        req(b"HEAD /a%2fb HTTP/1.0", (b"Accept-Language: en", b"host: [2001:db8::1]:443", b"Cookie: a=b; c=d")),
        req(b"PUT /u HTTP/1.1", (b"Content-Length: 3", b"Host: up.example", b"Expect: 100-continue"), eol=b"\n", body=b"abc"),
    ]
    for b in bases:
        e = http_ref.http_request_host(b)
        assert e[0] == 0 and e[1] > 0
    out = []
    for k in range(count):
        base = bases[k % len(bases)]
        head = base.index(b"\n\n") + 2 if b"\r" not in base else base.index(b"\r\n\r\n") + 4
        spots = [0, base.index(b"\n") - 1] + [base.index(b" ") + 1] * 3   # the uri's first byte decides its form
        at = 0
        while at < head:
            spots.append(at)
            colon = base.find(b":", at, base.index(b"\n", at))
            if colon >= 0:
                spots += [colon, colon + 1, colon + 2]
            at = base.index(b"\n", at) + 1
        pos = int(rng.choice(spots)) if rng.integers(0, 2) else int(rng.integers(0, head))
        kind = ("flip", "insert", "insert", "insert", "delete", "delete", "truncate", "flip")[int(rng.integers(0, 8))]
        m = bytearray(base)
        if kind == "flip":
            m[pos] ^= int(rng.integers(1, 256))
        elif kind == "insert":
            m.insert(pos, _FUZZ_BYTES[int(rng.integers(0, len(_FUZZ_BYTES)))])
        elif kind == "delete":
            del m[pos]
        else:
            del m[max(pos, 1):]
        out.append((f"fuzz{k}_{kind}_at{pos}", bytes(m)))
    return tuple(out)


def all_cases():
    return list(lattice_cases()) + list(window_cases()) + list(fuzz_cases())


def unrecognised():
    """Prefixes that are neither isHTTP nor isTLS, and ones too short to tell."""
    return (("unrec_empty", b""), ("unrec_1", b"G"), ("unrec_2_tls", b"\x16\x03"), ("unrec_zeros", bytes(40)),
            ("unrec_dash_third", b"SS-2.0\r\n"), ("unrec_digits", b"12345 / HTTP/1.1\r\n\r\n"),
            ("unrec_tls_major_4", b"\x16\x04\x01\x00\x02ab"), ("unrec_tls_type_18", b"\x18\x03\x01\x00\x02ab"),
            ("unrec_tls_minor_10", b"\x16\x03\x0a\x00\x02ab"), ("unrec_3_bytes", b"\x00\x01\x02"),
            ("unrec_high", b"\xff\xfe\xfd\xfc"))


@functools.lru_cache(maxsize=None)
def mixed_cases():
    """HTTP, TLS-record and unrecognised prefixes interleaved, so the waves of
    one workgroup take different branches."""
    http = list(lattice_cases()) + list(small_window_cases())[::3]
    tls = [x for x in sc.record_cases() if not x[0].startswith("rec_fuzz")]
    tls = tls[:70] + tls[-20:]
    other = list(unrecognised())
    out = []
    for k in range(max(len(http), len(tls))):
        out.append(http[k % len(http)])
        out.append(tls[k % len(tls)])
        if k % 3 == 0:
            out.append(other[(k // 3) % len(other)])
    return tuple((f"mix{k}_{n}", m) for k, (n, m) in enumerate(out))


def expected(cases, fn, stride=NAME_STRIDE):
    """[(status, name_len, name_off, need, name)] by the restatement."""
    return [fn(m, stride) for _, m in cases]


def small_templates():
    """Stream prefixes of 10 to 48 bytes for the batch above the grid cap."""
    t = [b"GET / HTTP/1.1\r\n\r\n", b"GET / HTTP/1.1\r\nHost: a\r\n\r\n", b"GET / HTTP/1.1\nHost: bc:80\n\n",
         b"GET / HTTP/1.1\r\nHost: d.e\r\n\r\n", b"GET / HTTP/1.1\r\nHost: f.gh:1\r\n\r\n", b"GET / HTTP/1.1\r\nnocolon\r\n\r\n",
         b"GET x HTTP/1.1\r\nHost: a\r\n\r\n", b"GET / HTTP/1.1\r\nHost: a\r\n", b"\x16\x03\x01\x00\x05hello", b"GET / HTTP/11\r\n\r\n",
         b"GET / HTTP/1.1\r\nHost: abcde\r\n\r\n"]
    assert all(10 <= len(x) <= 48 for x in t)
    return t
