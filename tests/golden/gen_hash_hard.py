"""Writes tests/golden/hash_hard_messages.json: per length of tests/hash_cases.py: HARD17_LENGTHS the first candidate message
(hash_cases.hard_candidate(index, length)) whose first passing counter is >= 16, found with the module's restated filter (hashlib, the
range rules, Euler's criterion).  3.6e-5 of the messages are that hard: some 28 000 candidates per length on average, minutes of plain
Python in all (one process per length).  The file holds the tag, the index, the length and the claimed try count — no bytes of any
message; tests/test_hash_cases.py recomputes every entry from the oracles.
Run from the repository root: python tests/golden/gen_hash_hard.py"""
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import hash_cases as hc  # noqa: E402


def search(length):
    index, tries = hc.find_hard(length, 17)
    return {"tag": hc.HARD_TAG, "index": index, "length": length, "tries": tries}


if __name__ == "__main__":
    with multiprocessing.Pool(min(len(hc.HARD17_LENGTHS), os.cpu_count() or 1)) as pool:
        found = pool.map(search, hc.HARD17_LENGTHS)
    with open(hc.FIXTURE, "w") as f:
        json.dump({"min_tries": 17, "messages": found}, f, indent=1)
        f.write("\n")
