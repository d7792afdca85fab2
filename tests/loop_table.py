"""The operand contract of libsslam_loop.so as a table, as tests/graph_table.py is for libsslam_graph.so: for every entry that takes
device pointers, the least alignment in bytes of each pointer argument - what the block "ALIGNMENT" of include/sslam_loop.h
states, line for line - and the size limits - what its block "SIZE LIMITS" states, line for line (tests/test_loop_cpu.py compares
both and holds the table against sslam_amd.lib.LOOP_EXPORTS and the library's dynamic symbols; tests/test_gpu_loop.py runs every
row at its loosest alignment).  No entry of this library takes a stride.
No torch, no GPU: importable anywhere.
"""

E_INVALID, E_UNSUPPORTED = -1, -2
MAX_FRAMES, MAX_K, MAX_PER_FRAME = 4096, 4096, 8
MAX_NODES, MAX_EDGES, MAX_GRAPHS, MAX_ITER, MAX_CG = 4096, 65536, 65535, 16, 4096

# entry -> {pointer argument: least alignment in bytes}, in the header's order
ALIGN = {
    "ssll_frame_signatures": dict(desc=4, scores=4, workspace=4, sig=4),
    "ssll_loop_candidates": dict(sig=16, first=4, second=4, sim=4, count=4),
    "ssll_pose_graph_sparse": dict(edge_first=4, edge_second=4, edge_T=8, edge_info=8, C_in=8, workspace=8, C=8, status=4, iterations=4,
                                   used_edges=4, skipped_edges=4, failed_row=4, cost_in=8, cost=8, edge_chi2=8, cg_steps=4),
}

# entry -> the expressions the dispatch code tests (each with the code returned where it is false), the largest accepted value of
# each limited argument, and the widths in bits of the kernels' index expressions
LIMITS = {
    "ssll_frame_signatures": dict(limits=[("n_frames <= 4096", E_UNSUPPORTED), ("k <= 4096", E_UNSUPPORTED),
                                          ("d == 128 or d == 256", E_UNSUPPORTED)],
                                  largest=dict(n_frames=MAX_FRAMES, k=MAX_K, d=256), widths={"frame * k * d": 64}),
    "ssll_loop_candidates": dict(limits=[("n_frames <= 4096", E_UNSUPPORTED), ("d == 128 or d == 256", E_UNSUPPORTED),
                                         ("per_frame <= 8", E_UNSUPPORTED)],
                                 largest=dict(n_frames=MAX_FRAMES, d=256, per_frame=MAX_PER_FRAME),
                                 widths={"frame * d": 31, "frame * per_frame": 31}),
    "ssll_pose_graph_sparse": dict(limits=[("n_nodes <= 4096", E_UNSUPPORTED), ("n_edges <= 65536", E_UNSUPPORTED),
                                           ("n_graphs <= 65535", E_UNSUPPORTED), ("cg_iterations <= 4096", E_UNSUPPORTED)],
                                   largest=dict(n_nodes=MAX_NODES, n_edges=MAX_EDGES, n_graphs=MAX_GRAPHS, cg_iterations=MAX_CG),
                                   widths={"graph * n_edges * 21": 64, "graph * workspace doubles": 64, "slot * 90": 31}),
}

# the entries that take no device pointer
HOST_ONLY = ["ssll_version", "ssll_arch", "ssll_launch_count", "ssll_pose_graph_sparse_workspace_bytes"]


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


def signature_workspace_bytes(n_frames, d):
    return 4 * n_frames * d


def sparse_workspace_bytes(n_graphs, n_nodes, n_edges):
    return 8 * n_graphs * (90 * n_edges + 78 * (n_nodes - 1) + 12 * n_nodes + (n_nodes + 1 + 2 * n_edges + 1) // 2)
