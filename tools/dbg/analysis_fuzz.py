#!/usr/bin/env python3
"""Differential fuzz of the dense-tensor analyses on the GPU against their numpy restatements: the generator of
tests/_analysis_fuzz.py at any seed and any number of mix cases an analysis. Every case asserts written / alone / reference
(tests/_analysis_fuzz.py, drive); the first failing case is printed as the tuple `_analysis_fuzz.Case(*tuple)` rebuilds, then the
run goes on with the next analysis. usage (GPU box): python tools/dbg/analysis_fuzz.py [seed] [mix cases an analysis] [analysis ...]"""
import dataclasses, os, sys, time, traceback
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    per = int(sys.argv[2]) if len(sys.argv) > 2 else None
    only = sys.argv[3:]
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    import _analysis_fuzz as FZ
    from foldcomp_amd.codec import Codec
    failed, done, t0 = {}, 0, time.time()
    with Codec(0) as codec:
        for case in FZ.cases(seed, per):
            if (only and case.analysis not in only) or case.analysis in failed:
                continue
            t = time.time()
            try:
                b = FZ.drive(codec, case)
            except AssertionError:
                failed[case.analysis] = case
                print(f"FAILED {case.id}\n  rebuild with _analysis_fuzz.Case(*{dataclasses.astuple(case)!r})")
                traceback.print_exc(limit=4)
                continue
            done += 1
            print(f"ok {case.id:28s} {case.form!s:22s} n = {len(case.lens)}, rows = {sum(case.lens)}, redrawn {b.redrawn}, loose {b.loose}, {time.time() - t:.2f} s", flush=True)
    print(f"seed {seed}: {done} cases passed, {len(failed)} analyses failed ({', '.join(failed) or 'none'}), {time.time() - t0:.1f} s")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
