"""calitas_find_edit_sites timed on one contig of the bench genome recipe (bench.build_genome), alone on the chip, in ONE process:
python tools/edit_sites_speed.py [contig index = 20] [rounds = 5]

For N20 + nrg, a C->T editor (install) with the window 3:8 and with the window over the whole protospacer, and 10^5 and 10^7 editor
targets at random positions of the contig (a C becomes T, a G becomes A; ref not given), these arms:

  count   : calitas_count_edit_sites (the SNVs uploaded, the count kernel, the counters and the status bytes back)
  list    : calitas_find_edit_sites (the same, the scan of the workgroups' sums, the write kernel, the records copied back once);
            left out, and said so, where the records are more than 2^26 (two gigabytes)
  allele  : calitas_count_allele_sites on the same SNVs, the yardstick: the edit count matches one allele on one strand, the allele
            count two alleles on both
  twin    : calitas_find_edit_sites_host over the same SNVs, once; left out above 10^5 SNVs.  Held against the device's records byte
            for byte.

One contig, as tools/allele_sites_speed.py measures: a lane's loads are scattered over 46.7 Mb of text (17.5 MB of planes and mask),
far more than the caches next to the compute units hold, so the whole genome resident would add the minute it takes to build and
nothing to what a lane waits for.

A call is timed by the host clock around the library call, blocks freed inside it and the library's deferred frees waited for
(calitas_reap_wait).  Every device arm is first called once (it sizes the buffers), then median / min / max over the rounds; the host arm
runs once.  No ratio is a pass criterion."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (100000, 10000000)
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
    made = np.zeros(256, dtype="S1")                            # the SNV the editor makes of a letter, "" where it makes none
    for ref, alt in (("C", "T"), ("G", "A")):
        made[ord(ref)] = made[ord(ref.lower())] = alt.encode()
    fits = np.flatnonzero(made[text] != b"")                     # the contig's C and G

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

    def show(size, window, arm, t, note=""):
        print("%-9d %-5s %-6s median %10.2f ms  min %10.2f  max %10.2f  %s" % (size, window if isinstance(window, str) else "%d:%d" % window, arm, t[len(t) // 2], t[0], t[-1], note), flush=True)

    rng = np.random.default_rng(7)
    for size in SIZES:
        snvs = np.zeros(size, dtype=C.SNV_DTYPE)
        pos = fits[rng.integers(0, len(fits), size=size)]
        snvs["position"] = pos
        snvs["alt"] = made[text[pos]]
        for window in ((3, 8), (0, 20)):
            edit = C.BaseEdit("C", "T", window)
            (n, by, status), t = timed(lambda: ctx.count_edit_sites(pat, edit, snvs), rounds)
            show(size, window, "count", t, "%d records: %s with 0 / 1 / 2 / 3+ bystanders; status 0 .. 5: %s" %
                 (n, " / ".join(str(int(x)) for x in by), " / ".join(str(int((status == k).sum())) for k in range(6))))
            got = None
            if n <= MOST_RECORDS:
                got, t = timed(lambda: ctx.find_edit_sites(pat, edit, snvs), rounds)
                assert len(got) == n
                show(size, window, "list", t, "%.1f MB of records" % (n * 32 / 1e6))
            else:
                print("%-9d %-5s list   left out: %d records" % (size, "%d:%d" % window, n), flush=True)
            if size <= MOST_TWIN:
                twin, t = timed(lambda: ctx.find_edit_sites(pat, edit, snvs, host=True), 0)
                assert got is not None and twin.sites.tobytes() == got.sites.tobytes() and twin.status.tobytes() == got.status.tobytes(), "device and twin differ"
                show(size, window, "twin", t)
            else:
                print("%-9d %-5s twin   left out" % (size, "%d:%d" % window), flush=True)
        (n, by, status), t = timed(lambda: ctx.count_allele_sites(pat, snvs), rounds)
        show(size, "-", "allele", t, "%d records" % n)
    ctx.close()


if __name__ == "__main__":
    main()
