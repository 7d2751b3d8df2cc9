"""hysteria_amd -- Hysteria's Salamander packet obfuscation (extras/obfs) on AMD MI355X.

The product is ``libhyobfs.so`` (gfx950 HIP kernels behind the C ABI of
``include/hyobfs.h``); this package is its Python host binding.
"""
from . import acl, addr, gecko, request, sniff, udpmsg  # noqa: F401
from .acl import (  # noqa: F401
    ACL_RESULT_DTYPE,
    CompilationError,
    InvalidSyntaxError,
    RuleSet,
    TextRule,
    compile_rules,
    parse_text_rules,
    quic_sniff_and_match,
)
from .addr import AddrError, relay_acl_decisions  # noqa: F401
from .request import PortSet, RequestError, hooked_relay_acl_decisions, tcp_request_decisions  # noqa: F401
from .conn import SalamanderPacketConn, wrap_packet_conn_salamander  # noqa: F401
from .gecko import GeckoOptions, GeckoPacketConn, GeckoReceiver, wrap_packet_conn_gecko  # noqa: F401
from .salamander import (  # noqa: F401
    BATCH_MAX_DATAGRAM,
    SM_KEY_LEN,
    SM_PSK_MIN_LEN,
    SM_SALT_LEN,
    UDP_BUFFER_SIZE,
    PSKTooShortError,
    SalamanderObfuscator,
    build_id,
    deobfuscate_batch_sharded,
    device_count,
    device_pci_bus_id,
    new_salamander_obfuscator,
    obfuscate_batch_sharded,
    synth_bimodal_lengths,
    synth_stream,
    synth_u64,
    workspace_size,
)
from .sniff import (  # noqa: F401
    SNIFF_RESULT_DTYPE,
    SniffError,
    Sniffer,
    client_hello_sni_batch,
    http_request_host_batch,
    quic_sniff_batch,
    tcp_sniff_batch,
    tls_record_sni_batch,
)

from .udpmsg import (  # noqa: F401
    UDP_META_DTYPE,
    UDP_PARSED_DTYPE,
    Defragger,
    UDPMessage,
    UDPMessageError,
    frag_udp_message,
    parse_udp_message,
    relay_quic_snis,
)

__all__ = [
    "SM_KEY_LEN", "SM_PSK_MIN_LEN", "SM_SALT_LEN", "UDP_BUFFER_SIZE", "PSKTooShortError",
    "SalamanderObfuscator", "device_count", "device_pci_bus_id", "new_salamander_obfuscator", "synth_bimodal_lengths",
    "synth_stream", "synth_u64", "workspace_size", "SalamanderPacketConn", "wrap_packet_conn_salamander",
    "obfuscate_batch_sharded", "deobfuscate_batch_sharded", "gecko", "GeckoOptions", "GeckoPacketConn",
    "wrap_packet_conn_gecko", "build_id", "sniff", "Sniffer", "SniffError", "SNIFF_RESULT_DTYPE",
    "client_hello_sni_batch", "tls_record_sni_batch", "quic_sniff_batch", "acl", "ACL_RESULT_DTYPE", "CompilationError",
    "InvalidSyntaxError", "RuleSet", "TextRule", "compile_rules", "parse_text_rules", "quic_sniff_and_match",
    "http_request_host_batch", "tcp_sniff_batch", "BATCH_MAX_DATAGRAM", "udpmsg", "UDPMessage", "UDPMessageError",
    "parse_udp_message", "frag_udp_message", "Defragger", "relay_quic_snis", "UDP_PARSED_DTYPE", "UDP_META_DTYPE",
    "GeckoReceiver", "addr", "AddrError", "relay_acl_decisions", "request", "PortSet", "RequestError",
    "tcp_request_decisions", "hooked_relay_acl_decisions",
]
