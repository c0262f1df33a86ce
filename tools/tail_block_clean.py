#!/usr/bin/env python3
"""Analysis tooling (CPU, the oracle): how many of a solve's block rounds (17 <= K <= 192 bidders) are clean -- every bidder
on a different object, every object bid on owned --, split at K = 64 (profiles/tail_block_clean.txt).
usage: tail_block_clean.py [config ...]"""
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from sslap_amd import synth
from _tail_block_clean import count_clean

for cfg in sys.argv[1:] or ["C2", "C3"]:
    loc, val = synth.gen_config(cfg)
    c = count_clean(loc, val, "max")
    tot = [c["K<=64"][k] + c["K>64"][k] for k in range(4)]
    print(json.dumps({"cfg": cfg, "rounds": c["rounds"], "columns": ["block rounds", "clean", "contested", "chain end"],
                      "K<=64": c["K<=64"], "K>64": c["K>64"], "all": tot,
                      "clean_share": round(tot[1] / max(tot[0], 1), 4)}), flush=True)
