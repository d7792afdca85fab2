"""The operand contract of libsslam_window.so as a table, as tests/graph_table.py is for libsslam_graph.so: for the entry that takes
device pointers, the least alignment in bytes of each pointer argument - what the block "ALIGNMENT" of include/sslam_window.h
states, line for line - and the size limits - what its block "SIZE LIMITS" states, line for line (tests/test_window_cpu.py compares
both and holds the table against sslam_amd.lib.WINDOW_EXPORTS and the library's dynamic symbols; tests/test_gpu_window.py runs every
row at its loosest alignment).  No entry of this library takes a stride.
No torch, no GPU: importable anywhere.
"""

E_INVALID, E_UNSUPPORTED = -1, -2
MAX_WINDOW, MAX_SPACINGS, MAX_WINDOWS, MAX_FRAME, MAX_ITER = 32, 8, 65535, 2 ** 31 - 2, 16
MAX_CAPACITY = 0x7fffffffffffffff // 96      # at n_windows = 1

# entry -> {pointer argument: least alignment in bytes}, in the header's order
ALIGN = {
    "sslw_window_step": dict(t=4, ring_first=4, ring_second=4, ring_T=8, ring_info=8, ring_C=8, trajectory=8, spacings=4, new_T=8, new_info=8,
                             new_status=4, new_inliers=4, C_start=8, workspace=8, C_window=8, base=4, n_nodes=4, admitted=4, predicted_from=4,
                             lost=4, status=4, iterations=4, used_edges=4, dropped_edges=4, failed_row=4, cost_in=8, cost=8, edge_chi2=8),
}
MAY_BE_NULL = ("C_start",)

# entry -> the expressions the dispatch code tests (each with the code returned where it is false), the largest accepted value of
# each limited argument, and the widths in bits of the kernel's index expressions
LIMITS = {
    "sslw_window_step": dict(limits=[("window <= 32", E_UNSUPPORTED), ("n_spacings <= 8", E_UNSUPPORTED), ("n_windows <= 65535", E_UNSUPPORTED),
                                     ("capacity <= 0x7fffffffffffffff / 96 / n_windows", E_UNSUPPORTED)],
                             largest=dict(window=MAX_WINDOW, n_spacings=MAX_SPACINGS, n_windows=MAX_WINDOWS, capacity=MAX_CAPACITY),
                             widths={"window * capacity * 12": 64, "window * workspace doubles": 64, "frame * 12": 64, "row * (row + 1) / 2": 31}),
}

# the entries that take no device pointer
HOST_ONLY = ["sslw_version", "sslw_arch", "sslw_launch_count", "sslw_window_workspace_bytes"]


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


def workspace_bytes(n_windows, window, n_spacings):
    return 8 * n_windows * (24 * window + 256 * 90 + window * n_spacings)


def lds_bytes(window):
    """The dynamic LDS of a launch: the lower triangle of A, then g, y and delta."""
    n = 6 * (window - 1)
    return 8 * (n * (n + 1) // 2 + 3 * n)
