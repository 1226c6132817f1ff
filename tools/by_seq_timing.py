"""End-to-end wall time of `dashing-amd dist_by_seq --nearest-neighbors 10` over one ~100 MB FASTA of 100 000 x 1 kbp
records at p = 10 (three runs; one JSON line)."""
import json
import os
import subprocess
import tempfile
import time

import numpy as np

d = tempfile.mkdtemp(dir=os.environ.get("TMPDIR", "/tmp"))
fa = os.path.join(d, "recs.fa")
rng = np.random.default_rng(1)
L = np.frombuffer(b"ACGT", np.uint8)
with open(fa, "wb") as f:
    for i in range(100):
        blk = L[rng.integers(0, 4, 1000 * 1000)].reshape(1000, 1000)
        f.write(b"".join(b">r%d\n" % (i * 1000 + j) + blk[j].tobytes() + b"\n" for j in range(1000)))
cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dashing_amd", "dashing-amd")
res = {"input_bytes": os.path.getsize(fa), "records": 100000, "length": 1000, "p": 10}
for rep in range(3):
    t0 = time.perf_counter()
    r = subprocess.run([cli, "dist_by_seq", "-S", "10", "-p", "16", "--nearest-neighbors", "10", "-O", os.path.join(d, "nn.tsv"), "-o", os.devnull, fa], capture_output=True, timeout=600)
    res.setdefault("wall_s", []).append(time.perf_counter() - t0)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
res["nn_lines"] = sum(1 for _ in open(os.path.join(d, "nn.tsv")))
print(json.dumps(res))
