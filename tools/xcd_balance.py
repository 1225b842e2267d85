"""Per-XCD balance of the fast matcher's launches, from a -DPGICP_XCC_STATS build (STATS=-DPGICP_XCC_STATS tools/stats_build.sh,
or such a library through PGICP_LIB_OVERRIDE):

    PGICP_PHASE_EACH_PASS=1 python3 bench.py --gpus 1 --steps 1 --warmup 1 2> err.txt
    python3 tools/xcd_balance.py err.txt [label]

Every matcher pass of that build prints, per hardware XCC (the XCC_ID register), when its last wave of k_knn_grid ended after
the launch's first wave began, its waves' time summed, its waves, and those waves by blockIdx.x & 7.  This prints, for the
launches of the LAST step in the file: the XCDs' end times, max / mean of them, each XCD's idle share (1 - its end / the last
end), max / mean of the summed wave time (the load itself, whatever the dispatcher made of it), and once which block class
each XCC ran.  Ticks are 10 ns (the 100 MHz clock all XCDs share)."""
import re
import sys


def parse(path):
    steps, cur = [], None
    for line in open(path, errors="replace"):
        m = re.search(r"fast kernel per XCC \(seeded (\d+)\)", line)
        if not m:
            continue
        seeded = int(m.group(1))
        cells = re.findall(r"(\d+)\|(\d+)\|(\d+)\|([\d,]+)", line.split("ticks of 10 ns:")[1])
        x = [(int(a), int(b), int(c), [int(v) for v in d.split(",")]) for a, b, c, d in cells]
        if seeded == 0 or cur is None:
            cur = []
            steps.append(cur)
        cur.append((seeded, x))
    return steps


def main():
    steps = parse(sys.argv[1])
    label = sys.argv[2] if len(sys.argv) > 2 else sys.argv[1]
    if not steps:
        sys.exit("no per-XCC lines: not a PGICP_XCC_STATS build, or PGICP_PHASE_EACH_PASS unset")
    print(f"== {label}: {len(steps)} step(s) in the file, the last one has {len(steps[-1])} fast-matcher launches")
    classes = [max(range(8), key=lambda c: x[3][c]) if x[2] else -1 for x in steps[-1][0][1]]
    pure = all(x[3][c] == x[2] for x, c in zip(steps[-1][0][1], classes) if x[2])
    print(f"block class (blockIdx.x & 7) run by XCC 0..7: {classes}" + (" -- every wave of an XCC from that one class" if pure else " -- MIXED: " + str([x[3] for x in steps[-1][0][1]])))
    print("launch seeded | end of each XCC after the launch's first wave, us | max/mean end | idle share of each XCC, % | max/mean wave time | waves")
    for k, (seeded, x) in enumerate(steps[-1]):
        live = [c for c in x if c[2]]
        ends = [c[0] / 100.0 for c in x]
        work = [c[1] for c in live]
        last = max(ends)
        mean_end = sum(c[0] for c in live) / 100.0 / len(live)
        print(f"{k:2d} {seeded} | " + " ".join(f"{e:7.1f}" for e in ends) + f" | {last / mean_end:.3f} | " +
              " ".join(f"{100.0 * (1.0 - e / last):4.1f}" for e in ends) + f" | {max(work) * len(work) / sum(work):.3f} | {sum(c[2] for c in x)}")


if __name__ == "__main__":
    main()
