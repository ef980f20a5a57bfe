"""bench.py on the GPU: a plain run is the headline alone, and --dump-outputs
writes the embedding rows its last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bertpy
from conftest import ROOT

pytestmark = pytest.mark.gpu

ARCH, FTYPE, B, L, SEED = "all-MiniLM-L6-v2", "f16", 5, 33, 1234
FULL_ONLY = ("hbm", "library_path", "encode_path", "cpu_baseline", "probes")


@pytest.fixture(scope="module", autouse=True)
def _one_device():
    os.environ.pop("BERT_HOST_ONLY", None)
    os.environ["BERT_DEVICES"] = "0"


def test_plain_run_is_the_headline_alone_and_dumps_its_outputs(tmp_path):
    models, dump = str(tmp_path / "models"), str(tmp_path / "dump")
    env = dict(os.environ)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--arch", ARCH, "--ftype", FTYPE, "--batch", str(B), "--seq", str(L), "--seed", str(SEED),
                        "--model-dir", models, "--dump-outputs", dump],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [x for x in r.stdout.decode().splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()
    res = json.loads(lines[0])
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0 and res["full"] is False
    assert abs(res["value"] - B * 1e3 / res["ms_per_step"]) / res["value"] < 1e-3
    assert not [k for k in FULL_ONLY if k in res] and res["roofline"] is None and res["kernels"] == {}
    assert os.listdir(dump) == ["embeddings.npy"]
    got = np.load(os.path.join(dump, "embeddings.npy"))
    assert got.dtype == np.float32 and got.shape == (B, bertpy.ARCHS[ARCH]["n_embd"])
    # the same model file and the same seeded ids through the library's host-buffer
    # entry: the graph the device-resident entry replays, so the rows agree bitwise
    ids = bertpy.synthetic_ids(B, L, bertpy.ARCHS[ARCH]["n_vocab"], seed=7)
    ref = bertpy.BertModel(os.path.join(models, f"{ARCH}-{FTYPE}-seed{SEED}.bin")).forward_batch(ids)
    assert np.array_equal(got, ref)
