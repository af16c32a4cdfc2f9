"""The cost of a context's lifetime, measured from the host: create + close of a 64-slot context (length 40, 32768 points), eight cycles
per repetition.
   python tools/context_cycles.py [repetitions]   -> JSON (ms per repetition of eight cycles: median, min, max, all)"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from groundgrid_amd import api


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    api.GroundSegmentation().init(40.0, 0.33, n_slots=64, max_points=32768).close()  # (the runtime's own first-use costs)
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(8):
            api.GroundSegmentation().init(40.0, 0.33, n_slots=64, max_points=32768).close()
        ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    print(json.dumps({"lib": os.environ.get("GROUNDGRID_HIP_LIB", "default"), "eight_cycles_ms_median": statistics.median(ms), "eight_cycles_ms_min": min(ms),
                      "eight_cycles_ms_max": max(ms), "eight_cycles_ms": ms}))


if __name__ == "__main__":
    main()
