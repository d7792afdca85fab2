"""The operand contract of libsslam_conf.so as a table, as tests/place_table.py is for libsslam_place.so: for the entries that take
device pointers, the least alignment in bytes of each pointer argument - what the block "ALIGNMENT" of include/sslam_conf.h
states, line for line - and the size limits - what its block "SIZE LIMITS" states, line for line (tests/test_confidence_cpu.py
compares both and holds the table against sslam_amd.lib.CONF_EXPORTS and the library's dynamic symbols;
tests/test_gpu_confidence.py runs every row at its loosest alignment).  No entry of this library takes a stride.
No torch, no GPU: importable anywhere.
"""

E_INVALID, E_UNSUPPORTED = -1, -2
DINO_DIM, HIDDEN_DIM, FILTER_MAX_K, TILE_ROWS = 384, 128, 4096, 32

# entry -> {pointer argument: least alignment in bytes}, in the header's order
ALIGN = {
    "sslc_confidence_rows": dict(x=16, desc=16, packed=16, conf=4),
    "sslc_gather_confidence": dict(feat=16, kp_xy=4, desc=16, packed=16, conf=4),
    "sslc_confidence_filter": dict(conf=4, slot=4, count=4, conf_out=4),
    "sslc_take_rows": dict(src=4, slot=4, dst=4),
}

# entry -> the expressions the dispatch code tests (each with the code returned where it is false), the largest accepted value of
# each limited argument, and the widths in bits of the kernels' index expressions
LIMITS = {
    "sslc_confidence_rows": dict(limits=[("rows <= 0x7fffffff", E_UNSUPPORTED), ("D == 128 or D == 256", E_UNSUPPORTED)],
                                 largest=dict(rows=0x7fffffff, D=256),
                                 widths={"row * 384": 64, "row * D": 64, "tile = rows / 32": 31}),
    "sslc_gather_confidence": dict(limits=[("n_frames * K <= 0x7fffffff", E_UNSUPPORTED), ("D == 128 or D == 256", E_UNSUPPORTED)],
                                   largest=dict(rows=0x7fffffff, D=256),
                                   widths={"frame * G * G * 384": 64, "row * D": 64, "tile = rows / 32": 31}),
    "sslc_confidence_filter": dict(limits=[("K <= 4096", E_UNSUPPORTED)], largest=dict(K=FILTER_MAX_K), widths={"frame * K": 64}),
    "sslc_take_rows": dict(limits=[("n_frames * K * width <= 0x7fffffff", E_UNSUPPORTED)], largest=dict(words=0x7fffffff),
                           widths={"word index n_frames * K * width": 64}),
}

# the entries that take no device pointer
HOST_ONLY = ["sslc_version", "sslc_arch", "sslc_launch_count", "sslc_confidence_layout", "sslc_confidence_pack_host"]


def header_lines():
    """The ALIGNMENT table as the lines of the header's block: `entry: arg a, arg a, ...`."""
    return [f"{entry}: " + ", ".join(f"{k} {v}" for k, v in args.items()) for entry, args in ALIGN.items()]


def limit_lines():
    """The SIZE LIMITS table as the lines of the header's block."""
    out = []
    for entry, row in LIMITS.items():
        tests = "; ".join(f"{expr}, else {'SSLAM_E_UNSUPPORTED' if code == E_UNSUPPORTED else 'SSLAM_E_INVALID'}" for expr, code in row["limits"])
        out.append(f"{entry}: {tests}. offsets: " + ", ".join(f"{k} {v}" for k, v in row["widths"].items()))
    return out


def packed_floats(d):
    """Floats of the packed head at descriptor width d: every part rounded up to a multiple of 4."""
    up = lambda n: (n + 3) // 4 * 4       # noqa: E731
    h = HIDDEN_DIM
    return sum(up(n) for n in (h * (DINO_DIM + d), h, (h // 2) * h, h // 2, h // 2, 1))
