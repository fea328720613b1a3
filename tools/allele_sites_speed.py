"""calitas_find_allele_sites timed on one contig of the bench genome recipe (bench.build_genome), alone on the chip, in ONE process:
python tools/allele_sites_speed.py [contig index = 20] [rounds = 5]

For N20 + nrg and 10^3, 10^5 and 10^7 SNVs at random positions of the contig (alt another letter than the reference's, ref not given),
these arms:

  count   : calitas_count_allele_sites (the SNVs uploaded, the count kernel, the counters and the status bytes back)
  list    : calitas_find_allele_sites (the same, the scan of the workgroups' sums, the write kernel, the records copied back once);
            left out, and said so, where the records are more than 2^26 (two gigabytes)
  twin    : calitas_find_allele_sites_host over the same SNVs, once; left out above 10^5 SNVs.  Held against the device's records byte
            for byte.
  today   : what a user does without the call, for the smallest size only: calitas_find_sites of the window [position - 63,
            position + 64) of every SNV, one call each (the reference allele's sites), and allele_sites_of, the contract in plain
            Python, over a 127-base cut of the contig for the join with the alt allele.

A call is timed by the host clock around the library call, blocks freed inside it and the library's deferred frees waited for
(calitas_reap_wait).  Every device arm is first called once (it sizes the buffers), then median / min / max over the rounds; the host arms
run once.  No ratio is a pass criterion."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (1000, 100000, 10000000)
MOST_RECORDS = 1 << 26
MOST_TWIN = 100000


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    contig = int(args[0]) if len(args) > 0 else 20
    rounds = int(args[1]) if len(args) > 1 else 5
    import numpy as np
    import torch
    import bench
    import calitas_amd as C
    lib = C._lib.lib
    names, seqs = bench.build_genome(1.0, torch.device("cuda", 0), contig_indices=[contig], guides=[bench.GUIDE0], log=None)
    ctx = C.Context(0)
    ctx.set_reference(names, seqs, genome_build="synthetic")
    text = np.frombuffer(memoryview(seqs[0]), dtype=np.uint8).copy()
    del seqs
    length = ctx.contig_lengths[0]
    print("contig %s, %d bases" % (names[0], length), flush=True)
    pat = C.Guide("N" * 20 + "nrg")
    code = np.full(256, 0, dtype=np.uint8)
    for k, ch in enumerate("ACGT"):
        code[ord(ch)] = code[ord(ch.lower())] = k
    letters = np.frombuffer(b"ACGT", dtype="S1")

    def timed(fn, n):
        out = []
        for r in range(n + 1):                                  # (one call of warm-up: buffers sized, clocks up)
            lib.calitas_reap_wait()
            t0 = time.perf_counter()
            got = fn()
            lib.calitas_reap_wait()
            if r >= 1 or n == 0:
                out.append((time.perf_counter() - t0) * 1e3)
        out.sort()
        return got, out

    def show(size, arm, t, note=""):
        print("%-9d %-6s median %10.2f ms  min %10.2f  max %10.2f  %s" % (size, arm, t[len(t) // 2], t[0], t[-1], note), flush=True)

    rng = np.random.default_rng(7)
    for size in SIZES:
        snvs = np.zeros(size, dtype=C.SNV_DTYPE)
        pos = rng.integers(0, length, size=size)
        snvs["position"] = pos
        snvs["alt"] = letters[(code[text[pos]] + rng.integers(1, 4, size=size)) % 4]
        (n, by, status), t = timed(lambda: ctx.count_allele_sites(pat, snvs), rounds)
        show(size, "count", t, "%d records: %d alt, %d ref, %d both; status 0 / 1 / 2 / 3: %s" %
             (n, by[1], by[2], by[3], " / ".join(str(int((status == k).sum())) for k in range(4))))
        got = None
        if n <= MOST_RECORDS:
            got, t = timed(lambda: ctx.find_allele_sites(pat, snvs), rounds)
            assert len(got) == n
            show(size, "list", t, "%.1f MB of records" % (n * 32 / 1e6))
        else:
            print("%-9d list   left out: %d records" % (size, n), flush=True)
        if size <= MOST_TWIN:
            twin, t = timed(lambda: ctx.find_allele_sites(pat, snvs, host=True), 0)
            assert got is not None and twin.sites.tobytes() == got.sites.tobytes() and twin.status.tobytes() == got.status.tobytes(), "device and twin differ"
            show(size, "twin", t)
        else:
            print("%-9d twin   left out" % size, flush=True)
        if size == SIZES[0]:
            t0 = time.perf_counter()
            n_ref = 0
            for p in pos.tolist():
                n_ref += len(ctx.find_sites(pat, chrom=0, start=max(0, p - 63), end=min(length, p + 64)))
            t_find = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            joined = 0
            for v in snvs:
                p = int(v["position"])
                lo = max(0, p - 63)
                cut = text[lo:min(length, p + 64)].tobytes().decode()
                records, _ = C.allele_sites_of([cut], pat, [(0, p - lo, "", v["alt"].decode())])
                joined += len(records)
            t_join = (time.perf_counter() - t0) * 1e3
            assert joined == n, "the Python join and the device differ"
            print("%-9d today  %10.2f ms find_sites of %d windows (%d sites) + %10.2f ms the join in Python = %.2f ms" %
                  (size, t_find, size, n_ref, t_join, t_find + t_join), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
