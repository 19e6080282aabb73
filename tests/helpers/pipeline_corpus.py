"""The access-log read buffer shared by tests/test_gpu_pipeline.py, tests/test_gpu_edge_kernels.py and tests/test_edge_models.py."""
import numpy as np

from loongcollector_amd import corpus


def access_log_buffer(n_lines, seed=5, trailing_newline=True):
    """n access-log lines for regex B; every 7th has the user agent the benchmark's filter keeps, every 11th is junk the parser
    cannot match, every 13th is empty"""
    rng = np.random.default_rng(seed)
    data, off, length = corpus.apache_batch(n_lines, "B", line_bytes=200, seed=seed, pool_lines=min(n_lines, 512))
    lines = [bytes(data[o:o + l]) for o, l in zip(off[:-1], length)]
    out = []
    for i, l in enumerate(lines):
        if i % 13 == 12:
            out.append(b"")
        elif i % 11 == 10:
            out.append(b"{\"level\": \"info\", \"msg\": \"not an access log %d\"}" % i)
        elif i % 7 == 6:
            head, _, _ = l.rpartition(b' "')
            out.append(head + b' "no-agent"')
        else:
            out.append(l)
    buf = b"\n".join(out)
    return buf + (b"\n" if trailing_newline else b""), int(rng.integers(0, 1 << 40))
