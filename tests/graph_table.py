"""The operand contract of libsslam_graph.so as a table, as tests/ext_table.py is for libsslam_ext.so: for every entry that takes
device pointers, the least alignment in bytes of each pointer argument - what the block "ALIGNMENT" of include/sslam_graph.h
states, line for line - and the size limits - what its block "SIZE LIMITS" states, line for line (tests/test_pose_graph_cpu.py
compares both and holds the table against sslam_amd.lib.GRAPH_EXPORTS and the library's dynamic symbols;
tests/test_gpu_pose_graph.py runs every row at its loosest alignment).  No entry of this library takes a stride.
No torch, no GPU: importable anywhere.
"""

E_INVALID, E_UNSUPPORTED = -1, -2
MAX_BAND, MAX_NODES, MAX_EDGES, MAX_GRAPHS, MAX_ITER = 32, 4096, 1048576, 65535, 16

# entry -> {pointer argument: least alignment in bytes}, in the header's order
ALIGN = {
    "sslg_chain_poses": dict(T=8, C_start=8, C=8),
    "sslg_pose_graph": dict(edge_first=4, edge_second=4, edge_T=8, edge_info=8, C_in=8, workspace=8, C=8, status=4, iterations=4,
                            used_edges=4, skipped_edges=4, failed_row=4, cost_in=8, cost=8, edge_chi2=8),
}

# entry -> the expressions the dispatch code tests (each with the code returned where it is false), the largest accepted value of
# each limited argument, and the widths in bits of the kernel's index expressions
LIMITS = {
    "sslg_chain_poses": dict(limits=[("n_graphs <= 0x7fffffff / 256 and n_nodes <= 4096", E_UNSUPPORTED)],
                             largest=dict(n_graphs=0x7fffffff // 256, n_nodes=MAX_NODES), widths={"graph * n_nodes * 12": 64}),
    "sslg_pose_graph": dict(limits=[("band <= 32", E_UNSUPPORTED), ("n_nodes <= 4096", E_UNSUPPORTED), ("n_edges <= 1048576", E_UNSUPPORTED),
                                    ("n_graphs <= 65535", E_UNSUPPORTED)],
                            largest=dict(band=MAX_BAND, n_nodes=MAX_NODES, n_edges=MAX_EDGES, n_graphs=MAX_GRAPHS),
                            widths={"graph * n_edges * 21": 64, "graph * workspace doubles": 64, "row * (6 * band + 6)": 31}),
}

# the entries that take no device pointer
HOST_ONLY = ["sslg_version", "sslg_arch", "sslg_launch_count", "sslg_pose_graph_workspace_bytes"]


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


def workspace_bytes(n_graphs, n_nodes, band):
    n = 6 * (n_nodes - 1)
    return 8 * n_graphs * (n * (6 * band + 6) + 3 * n + 12 * n_nodes + 256 * 90)
