"""Condense the `ppo-tolerance` lines that tests/test_gpu_ppo.py prints (pytest -s) into the worst kernel / E_torch
ratio per input set and quantity: profiles/ppo_grad/tolerance.json.

    pytest tests/test_gpu_ppo.py -s -m gpu > log.txt;  python tools/ppo_tolerance.py log.txt profiles/ppo_grad/tolerance.json

Keys: "D=<obs_dim>" for the lines of test_ppo_grad_matches_the_reference (every B, normalisation and ent_coef of the
set; "D=1239 multi-stage" for its B >= 1000, where k_ppo_dw1 takes several stages per segment), and the label of
every other check (repeats, all once, permuted, out of range, collected ...), all of them at D = 29 or on the
collected rollout.  Values: {quantity: {kernel, e_torch, ratio}} of the line with the largest ratio.
"""
import ast
import json
import re
import sys


def main(src, dst):
    worst = {}
    for line in open(src):
        m = re.search(r"ppo-tolerance (.*?) (\{.*\})", line)
        if not m:
            continue
        label, figs = m.group(1), ast.literal_eval(m.group(2))
        shape = re.match(r"B=(\d+) D=(\d+) ", label)
        key = label
        if shape:
            key = f"D={shape.group(2)}" + (" multi-stage" if int(shape.group(1)) >= 1000 else "")
        for name, text in figs.items():
            a, rest = text.split("/")
            b, r = rest.split("=")
            r = 0.0 if r == "nan" else float(r)
            w = worst.setdefault(key, {})
            if name not in w or r >= w[name]["ratio"]:
                w[name] = dict(kernel=float(a), e_torch=float(b), ratio=r)
    with open(dst, "w") as fh:
        json.dump(worst, fh, indent=1)
    for key, w in worst.items():
        top = sorted(w.items(), key=lambda kv: -kv[1]["ratio"])[:3]
        print(key, [(k, v["ratio"]) for k, v in top])


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
