"""bench.py's own output: --dump-outputs (what the last timed step returned, as arrays) and what a plain run leaves to --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


@pytest.fixture(scope="module")
def hits_text():
    """A hits.txt of the oracle's on a small synthetic genome with planted sites: (text, header, rows, contig names)."""
    from calitas_amd import synth
    names, seqs = synth.make_genome([("chrA", 400000), ("chrB", 90000)], seed=11, guides=[("CTTGCCCCACAGGGCAGTAA", "nrg", False)],
                                    sites_per_guide=300, n_run_ends=200, n_block=1500)
    header, rows, _ = O.search_memory(names, [s.tobytes() for s in seqs], "CTTGCCCCACAGGGCAGTAAnrg", "x", d=5, p=1, g=2)
    text = ("\t".join(header) + "\n" + "".join("\t".join(r[c] for c in header) + "\n" for r in rows)).encode()
    assert len(rows) > 100
    return text, header, rows, names


def check_rows(text, names, arrays):
    """Every row of hits_rows is the row of the text that starts at its offset, its numbers those of the text's columns."""
    for r in arrays["hits_rows"]:
        off = int(r[0])
        assert text[off - 1:off] == b"\n"
        f = dict(zip(text[:text.index(b"\n")].decode().split("\t"), text[off:text.index(b"\n", off)].decode().split("\t")))
        want = [names.index(f["chromosome"]), int(f["coordinate_start"]), int(f["coordinate_end"]), 1 if f["strand"] == "+" else -1,
                float(f["allele_frequency"]) if f["allele_frequency"] else -1.0] + [int(f[c]) for c in bench.DUMP_COLUMNS[5:]]
        assert list(r[1:]) == want
    sample = bytes(arrays["hits_text"].astype(np.uint8))
    assert sample.endswith(b"\n") and all(b"\n" + ln + b"\n" in text for ln in sample.split(b"\n")[:-1])


def test_hits_arrays_every_row(hits_text):
    text, header, rows, names = hits_text
    a = bench.hits_arrays(text, len(rows), names)
    assert set(a) == {"hits_count", "hits_rows", "hits_text"}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert list(a["hits_count"]) == [len(rows), len(text)]
    assert a["hits_rows"].shape == (len(rows), 1 + len(bench.DUMP_COLUMNS))
    assert [int(x) for x in a["hits_rows"][:, 2]] == [int(r["coordinate_start"]) for r in rows]
    check_rows(text, names, a)
    assert 0 < len(a["hits_text"]) <= bench.DUMP_TEXT_BYTES


def test_hits_arrays_seeded_sample(hits_text):
    """Above max_rows the rows holding seeded byte offsets, and a text sample of at most max_text bytes: the same every time."""
    text, header, rows, names = hits_text
    a = bench.hits_arrays(text, len(rows), names, max_rows=40, max_text=3000)
    assert 10 < len(a["hits_rows"]) <= 40 and len(a["hits_text"]) <= 3000
    assert list(a["hits_rows"][:, 0]) == sorted(set(a["hits_rows"][:, 0]))
    check_rows(text, names, a)
    b = bench.hits_arrays(bytearray(text), len(rows), names, max_rows=40, max_text=3000)
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_write_outputs_keeps_to_its_budget(tmp_path):
    bench.write_outputs(str(tmp_path / "d"), {"x": np.zeros(4, dtype=np.float32)})
    assert np.load(str(tmp_path / "d" / "x.npy")).dtype == np.float32
    with pytest.raises(AssertionError):
        bench.write_outputs(str(tmp_path / "e"), {"x": np.zeros(9 << 20, dtype=np.float64)})


def test_dump_outputs_refuses_a_step_it_cannot_hold(tmp_path):
    """A guide batch frees its texts inside the step: --dump-outputs says so before it touches a GPU."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "4", "--dump-outputs", str(tmp_path / "d")],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "--dump-outputs" in out.stderr
    assert not (tmp_path / "d").exists()


@pytest.mark.gpu
def test_bench_plain_full_and_outputs(tmp_path):
    """A plain run prints the headline and nothing that needs work of its own; --full adds the CPU baseline and the parity sample;
    the outputs of two runs with the same arguments are the same arrays, and say what the result line says."""
    def run(*extra):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--scale", "0.01"]
                             + list(extra), capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])

    plain = run("--dump-outputs", str(tmp_path / "plain"))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in plain, k
    assert plain["steps"] == 3 and plain["ms_per_step"] > 0
    assert "cpu_baseline" not in plain and "parity_sample" not in plain
    full = run("--full", "--cpu-sample-mb", "4", "--dump-outputs", str(tmp_path / "full"))
    assert full["parity_sample"]["identical"] and full["parity_sample"]["rows"] > 0 and full["cpu_baseline"]["value"] > 0
    for name in ("hits_count", "hits_rows", "hits_text"):
        a, b = np.load(str(tmp_path / "plain" / (name + ".npy"))), np.load(str(tmp_path / "full" / (name + ".npy")))
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), name
    count = np.load(str(tmp_path / "plain" / "hits_count.npy"))
    assert list(count) == [plain["hits_per_pass"], plain["hits_bytes_per_pass"]]
    assert len(np.load(str(tmp_path / "plain" / "hits_rows.npy"))) == plain["hits_per_pass"]
