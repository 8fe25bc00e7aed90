"""Layout of the -DPGTG_STAMPS build's debug buffer (pgtg_env.hip STAMP / STAMPT / STAMPR), in 64-bit words, for
tools/stamps.py and tools/placement.py."""
SLOTS = 32              # STAMP: a row of 32 cycle stamps per wave, from word 0
TICK_BASE = 1 << 19     # STAMPT: a row per workgroup (< 2048) of k_envq<BIG, true> ...
TICK_ROW = 256          # ... of up to 256 wall-clock tick ends
REAL_BASE = 1 << 20     # STAMPR: a row per wave ...
REAL_ROW = 8            # ... of 8 wall-clock stamps (2: the wave's start, 3: its end)
