"""Condense the `ppo-step-tolerance` lines that tests/test_gpu_ppo_step.py prints (pytest -s; each line names the three
largest kernel / E_torch ratios of its call) into the worst ratio per input set: profiles/ppo_step/tolerance.json.

    pytest tests/test_gpu_ppo_step.py -s -m gpu > log.txt;  python tools/ppo_step_tolerance.py log.txt profiles/ppo_step/tolerance.json

Keys: "D=<obs_dim>" for pgtg_ppo_step (steps 1 and 7, clipped and not, the edge cases at D = 17 among them),
"adv_stats" for pgtg_ppo_adv_stats and "update drift" for Rollout.update with DeviceAdam against the float32 torch
loop's own drift.  Values: {quantity: {kernel, e_torch, ratio, line}} of the line with the largest ratio.
"""
import ast
import json
import re
import sys


def main(src, dst):
    worst = {}
    for line in open(src):
        m = re.search(r"ppo-step-tolerance (.*?) (\{.*\})", line)
        if not m:
            continue
        label, figs = m.group(1), ast.literal_eval(m.group(2))
        shape = re.match(r"D=(\d+) ", label)
        key = f"D={shape.group(1)}" if shape else ("adv_stats" if label.startswith("adv_stats") else label)
        for name, text in figs.items():
            a, rest = text.split("/")
            b, r = rest.split("=")
            r = 0.0 if r == "nan" else float(r)
            w = worst.setdefault(key, {})
            if name not in w or r >= w[name]["ratio"]:
                w[name] = dict(kernel=float(a), e_torch=float(b), ratio=r, line=label)
    with open(dst, "w") as fh:
        json.dump(worst, fh, indent=1)
    for key, w in worst.items():
        top = sorted(w.items(), key=lambda kv: -kv[1]["ratio"])[:3]
        print(key, [(k, v["ratio"]) for k, v in top])


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
