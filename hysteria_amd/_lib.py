"""ctypes binding of libhyobfs.so (include/hyobfs.h).

The library holds the gfx950 kernels; there is no CPU fallback.  If the .so is
missing or does not load, importing the product API raises immediately.
"""
from __future__ import annotations

import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HYOBFS_LIB") or os.path.join(_HERE, "libhyobfs.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "hyobfs.h")

HYOBFS_OK = 0
HYOBFS_ERR_PSK_TOO_SHORT = -1
HYOBFS_ERR_INVALID = -2
HYOBFS_ERR_HIP = -3
HYOBFS_ERR_NOMEM = -4
HYOBFS_ERR_NO_DEVICE = -5
HYOBFS_ERR_IO = -6
HYOBFS_ERR_CLOSED = -7
ABI_VERSION = 4   # the HYOBFS_ABI_VERSION these bindings are written for (include/hyobfs.h)


class HyobfsBatch(ctypes.Structure):
    """struct hyobfs_batch (include/hyobfs.h)."""

    _fields_ = [
        ("n", ctypes.c_uint64),
        ("in_", ctypes.c_void_p),
        ("in_off", ctypes.c_void_p),
        ("in_stride", ctypes.c_uint64),
        ("in_len", ctypes.c_void_p),
        ("len_uniform", ctypes.c_uint32),
        ("pkt_cap", ctypes.c_uint32),
        ("salts", ctypes.c_void_p),
        ("out", ctypes.c_void_p),
        ("out_cap", ctypes.c_uint64),
        ("out_stride", ctypes.c_uint64),
        ("out_off", ctypes.c_void_p),
        ("out_len", ctypes.c_void_p),
        ("out_total", ctypes.c_void_p),
        ("workspace", ctypes.c_void_p),
        ("workspace_bytes", ctypes.c_uint64),
    ]


class HyobfsDgram(ctypes.Structure):
    """struct hyobfs_dgram (include/hyobfs_conn.h)."""

    _fields_ = [
        ("buf", ctypes.c_void_p),
        ("len", ctypes.c_uint32),
        ("cap", ctypes.c_uint32),
        ("addr", ctypes.c_uint8 * 128),
        ("addrlen", ctypes.c_uint32),
        ("pad_", ctypes.c_uint32),
    ]


def header_functions(path: str = HEADER_PATH) -> list[str]:
    """Names of every function declared in include/*.h."""
    names = []
    inc = os.path.dirname(path)
    for fn in sorted(os.listdir(inc)):
        if not fn.endswith(".h"):
            continue
        text = open(os.path.join(inc, fn)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        names += re.findall(r"\b(hyobfs_[a-z0-9_]+)\s*\(", text)
    return sorted(set(names))


_vp, _sz, _u64, _u32, _i32, _i64 = (ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int,
                                     ctypes.c_int64)
_pbatch = ctypes.POINTER(HyobfsBatch)
_SIG = {   # include/hyobfs.h, include/hyobfs_conn.h: name -> (restype, argtypes)
    "hyobfs_abi_version": (_i32, []),
    "hyobfs_build_id": (ctypes.c_char_p, []),
    "hyobfs_status_string": (ctypes.c_char_p, [_i32]),
    "hyobfs_device_count": (_i32, []),
    "hyobfs_device_pci_bus_id": (_i32, [_i32, ctypes.c_char_p, _i32]),
    "hyobfs_salamander_new": (_i32, [_vp, _sz, _i32, ctypes.POINTER(_vp)]),
    "hyobfs_salamander_free": (None, [_vp]),
    "hyobfs_salamander_device": (_i32, [_vp]),
    "hyobfs_salamander_set_kernel": (_i32, [_vp, _i32]),
    "hyobfs_salamander_seed": (None, [_vp, _u64]),
    "hyobfs_salamander_next_salts": (None, [_vp, _vp, _sz]),
    "hyobfs_salamander_key": (_i32, [_vp, _vp, _vp]),
    "hyobfs_salamander_keys_batch": (_i32, [_vp, _vp, _vp, _u64, _vp]),
    "hyobfs_salamander_obfuscate": (_sz, [_vp, _vp, _sz, _vp, _vp, _sz]),
    "hyobfs_salamander_obfuscate_auto": (_sz, [_vp, _vp, _sz, _vp, _sz]),
    "hyobfs_salamander_deobfuscate": (_sz, [_vp, _vp, _sz, _vp, _sz]),
    "hyobfs_batch_workspace_size": (_u64, [_u64]),
    "hyobfs_batch_workspace_bytes": (_u64, [_pbatch]),
    "hyobfs_salamander_batch_kernel": (_i32, [_vp, _pbatch, _i32]),
    "hyobfs_salamander_obfuscate_batch": (_i32, [_vp, _pbatch, _vp]),
    "hyobfs_salamander_deobfuscate_batch": (_i32, [_vp, _pbatch, _vp]),
    "hyobfs_salamander_obfuscate_batch_sharded": (_i32, [_vp, _pbatch, _i32]),
    "hyobfs_salamander_deobfuscate_batch_sharded": (_i32, [_vp, _pbatch, _i32]),
    "hyobfs_shard_bounds": (_i32, [_vp, _u64, _i32, _vp]),
    "hyobfs_salamander_obfuscate_host": (_i32, [_vp, _pbatch, _u64]),
    "hyobfs_salamander_deobfuscate_host": (_i32, [_vp, _pbatch, _u64]),
    "hyobfs_host_alloc": (_vp, [_sz]),
    "hyobfs_host_free": (None, [_vp]),
    "hyobfs_conn_wrap": (_i32, [_i32, _vp, _u32, ctypes.POINTER(_vp)]),
    "hyobfs_conn_close": (_i32, [_vp]),
    "hyobfs_conn_free": (None, [_vp]),
    "hyobfs_conn_read_from": (_i64, [_vp, _vp, _sz, _vp, ctypes.POINTER(_u32)]),
    "hyobfs_conn_write_to": (_i64, [_vp, _vp, _sz, _vp, _u32]),
    "hyobfs_conn_read_batch": (_i32, [_vp, _vp, _u32]),
    "hyobfs_conn_write_batch": (_i32, [_vp, _vp, _u32]),
    "hyobfs_conn_set_coalescing": (_i32, [_vp, _u32, _u32]),
    "hyobfs_conn_flush": (_i32, [_vp]),
    "hyobfs_conn_set_read_deadline": (_i32, [_vp, _i64]),
    "hyobfs_conn_set_write_deadline": (_i32, [_vp, _i64]),
    "hyobfs_conn_stats": (_i32, [_vp, ctypes.POINTER(_u64)]),
    "hyobfs_synth_stream": (_i32, [_vp, _u64, _u64, _u64, _vp]),
    "hyobfs_synth_u64": (_i32, [_vp, _u64, _u64, _u64, _vp]),
    "hyobfs_synth_bimodal_lengths": (_i32, [_vp, _u64, _u64, _u64, _vp]),
}

_ACL_SIG = {   # include/hyobfs_acl.h (hysteria_amd/acl.py, which imports the sniffer's bindings and so cannot be
    # imported by them): load() declares these with the core table
    "hyobfs_acl_ruleset_new": (_i32, [_vp, _u32, _i32, ctypes.POINTER(_vp)]),
    "hyobfs_acl_ruleset_free": (None, [_vp]),
    "hyobfs_acl_ruleset_rules": (_u32, [_vp]),
    "hyobfs_acl_ruleset_bad_rule": (_i64, []),
    "hyobfs_acl_ruleset_new_flags": (_i32, [_vp, _u32, _i32, _u32, ctypes.POINTER(_vp)]),
    "hyobfs_acl_ruleset_bad_entry": (_i64, []),
    "hyobfs_acl_ruleset_new_opts": (_i32, [_vp, _u32, _i32, _vp, ctypes.POINTER(_vp)]),
    "hyobfs_acl_ruleset_entries": (_u32, [_vp]),
    "hyobfs_acl_ruleset_index_info": (_i32, [_vp, _u32, _vp]),
    "hyobfs_acl_regex_check": (_i32, [_vp, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_u32)]),
    "hyobfs_acl_regex_match": (_i32, [_vp, _u32, _vp, _u32]),
    "hyobfs_acl_match_batch": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp]),
    "hyobfs_acl_match_sniffed_batch": (_i32, [_vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp]),
}

_UDP_SIG = {   # include/hyobfs_udpmsg.h (hysteria_amd/udpmsg.py); declared by load() like the ACL's
    "hyobfs_udp_header_size": (_u32, [_u32]),
    "hyobfs_udp_serialize": (_i64, [_vp, _vp, _u32, _vp, _u32, _vp, _sz]),
    "hyobfs_udp_parse": (_i32, [_vp, _sz, _vp]),
    "hyobfs_udp_frag_plan": (_i32, [_u32, _u32, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_u32)]),
    "hyobfs_udp_send_frags": (_i32, [_vp, _vp, _vp, _u32, _vp, _sz, _vp, ctypes.POINTER(_u32)]),
    "hyobfs_udp_defragger_new": (_vp, []),
    "hyobfs_udp_defragger_free": (None, [_vp]),
    "hyobfs_udp_defragger_feed": (_i32, [_vp, _vp, _u64, _vp, ctypes.POINTER(_u32)]),
    "hyobfs_udp_parse_batch": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp]),
    "hyobfs_udp_frag_workspace_size": (_u64, [_u64]),
    "hyobfs_udp_frag_batch": (_i32, [_vp, _vp, _vp, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    "hyobfs_udp_assemble_batch": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
}

_u16p = ctypes.POINTER(ctypes.c_uint16)
_ADDR_SIG = {   # include/hyobfs_addr.h (hysteria_amd/addr.py); declared by load() like the ACL's
    "hyobfs_addr_split": (_i32, [_vp, _sz, ctypes.POINTER(_u32), ctypes.POINTER(_u32), ctypes.POINTER(_u32),
                                 ctypes.POINTER(_u32)]),
    "hyobfs_addr_parse_port": (_i32, [_vp, _sz, _u16p]),
    "hyobfs_addr_parse_ip": (_i32, [_vp, _sz, _vp]),
    "hyobfs_addr_parse": (_i32, [_vp, _sz, ctypes.POINTER(_u32), ctypes.POINTER(_u32), _vp, _vp,
                                 ctypes.POINTER(ctypes.c_uint8), _u16p]),
    "hyobfs_addr_format": (_i32, [_vp, _u32, ctypes.c_uint16, _vp, _sz]),
    "hyobfs_addr_parse_batch": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hyobfs_addr_parse_udp_batch": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hyobfs_addr_format_batch": (_i32, [_vp, _vp, _vp, _u64, _vp, _u64, _u64, _vp, _vp, _vp, _vp]),
}

_i64p, _u32p, _u8p = ctypes.POINTER(_i64), ctypes.POINTER(_u32), ctypes.POINTER(ctypes.c_uint8)
_REQ_SIG = {   # include/hyobfs_request.h (hysteria_amd/request.py); declared by load() like the ACL's
    "hyobfs_tcp_request_parse": (_i32, [_vp, _sz, _u32p, _u32p, _u32p, _u32p]),
    "hyobfs_tcp_request_build": (_i64, [_vp, _sz, _u32, _u64, _u64, _vp, _sz]),
    "hyobfs_tcp_response_parse": (_i32, [_vp, _sz, _u32p, _u8p, _u32p, _u32p, _u32p]),
    "hyobfs_tcp_response_build": (_i64, [_i32, _vp, _sz, _u32, _u64, _u64, _vp, _sz]),
    "hyobfs_req_padding_fill": (None, [_u64, _u64, _vp, _sz]),
    "hyobfs_port_union_parse": (_i32, [_vp, _sz, _vp, _u32, _u32p]),
    "hyobfs_port_union_contains": (_i32, [_vp, _i64, ctypes.c_uint16]),
    "hyobfs_sniff_check": (_i32, [_vp, _sz, _i32, _i32, _vp, _i64, _vp, _i64]),
    "hyobfs_request_rewrite": (_i64, [_vp, _sz, _i32, _vp, _sz, _i32, _vp, _sz, _u8p]),
    "hyobfs_portset_new": (_i32, [_vp, _u32, _i32, ctypes.POINTER(_vp)]),
    "hyobfs_portset_free": (None, [_vp]),
    "hyobfs_tcp_request_parse_batch": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hyobfs_sniff_check_batch": (_i32, [_vp, _vp, _vp, _vp, _u64, _i32, _i32, _vp, _vp, _vp]),
    "hyobfs_request_rewrite_batch": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _u64, _vp, _u64, _u64, _vp, _vp,
                                            _vp, _vp, _vp]),
    "hyobfs_tcp_response_build_batch": (_i32, [_vp, _vp, _vp, _vp, _vp, _u32, _vp, _u64, _u64, _vp, _u64, _vp, _vp,
                                               _vp]),
}

_lib = None
_variants = {}   # other builds loaded side by side (in-process A/B runs, scripts/ab_variants.py)


def declare(lib: ctypes.CDLL, tag: str, table: dict) -> ctypes.CDLL:
    """Set restype / argtypes of every function of ``table`` (name -> (restype,
    argtypes)) on ``lib``, once per CDLL and ``tag``.  An undeclared function
    would take its 64-bit arguments as C ints."""
    done = lib.__dict__.setdefault("_declared", set())
    if tag not in done:
        for name, (res, args) in table.items():
            f = getattr(lib, name)
            f.restype, f.argtypes = res, args
        done.add(tag)
    return lib


def load(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load libhyobfs.so and declare the ABI.  Raises OSError if it is missing.
    A different ``path`` loads that build beside the default one (each CDLL keeps
    its own symbols)."""
    global _lib
    if path == LIB_PATH and _lib is not None:
        return _lib
    if path != LIB_PATH and path in _variants:
        return _variants[path]
    if not os.path.exists(path):
        raise OSError(f"{path} is missing: build it with `make -C hysteria_amd/csrc` "
                      "(or __graft_entry__.build()); there is no CPU fallback")
    lib = ctypes.CDLL(path, use_errno=True)
    declare(lib, "core", _SIG)
    # a build without acl.hip (the emulated library of tests/emu/build.sh) still loads for what it
    # has; acl._alib() declares the table unconditionally, so using the ACL with such a build fails there
    if hasattr(lib, "hyobfs_acl_ruleset_new"):
        declare(lib, "acl", _ACL_SIG)
    if hasattr(lib, "hyobfs_udp_parse_batch"):   # likewise udpmsg.hip / udpmsg_host.cpp (udpmsg._ulib())
        declare(lib, "udpmsg", _UDP_SIG)
    if hasattr(lib, "hyobfs_addr_parse_batch"):   # likewise addr.hip / addr_host.cpp (addr._adlib())
        declare(lib, "addr", _ADDR_SIG)
    if hasattr(lib, "hyobfs_tcp_request_parse_batch"):   # likewise request.hip / request_host.cpp (request._rqlib())
        declare(lib, "request", _REQ_SIG)
    have = lib.hyobfs_abi_version()
    if have != ABI_VERSION:   # struct layouts and enum values differ between versions
        raise OSError(f"{path}: ABI version {have}, these bindings need {ABI_VERSION}: rebuild the library")
    if path == LIB_PATH:
        _lib = lib
    else:
        _variants[path] = lib
    return lib


def status_string(st: int) -> str:
    return load().hyobfs_status_string(st).decode()


class HyobfsError(RuntimeError):
    def __init__(self, status: int, what: str = ""):
        self.status = status
        super().__init__(f"{what}: {status_string(status)} ({status})" if what else status_string(status))


def check(status: int, what: str = "") -> None:
    if status != HYOBFS_OK:
        raise HyobfsError(status, what)
