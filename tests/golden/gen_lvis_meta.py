#!/usr/bin/env python3
"""The LVIS v0.5 category table as data: per class the name the REFERENCE's metadata gives it
(``_get_lvis_instances_meta_v0_5``: ``synonyms[0]`` of the categories sorted by id, groundingdino/datasets/builtin_meta.py), its
contiguous 0-based index (id - 1, what ``load_filtered_lvis_json`` maps annotations to) and its frequency letter ("r" rare, "c"
common, "f" frequent -- what LVISEval's APr / APc / APf group by).  Only the category module is imported: it holds nothing but
the lists.  Writes lvis_v0_5_categories.json beside this file: names, indices, letters and their counts, no program text.
      python tests/golden/gen_lvis_meta.py
"""
import collections
import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


def main():
    spec = importlib.util.spec_from_file_location(
        "lvis_v0_5_categories", os.path.join(REF, "groundingdino", "datasets", "lvis_v0_5_categories.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cats = sorted(mod.LVIS_CATEGORIES, key=lambda k: k["id"])
    assert len(cats) == 1230 and [k["id"] for k in cats] == list(range(1, 1231))
    rows = [{"index": k["id"] - 1, "name": k["synonyms"][0], "frequency": k["frequency"]} for k in cats]
    counts = collections.Counter(r["frequency"] for r in rows)
    assert set(counts) == {"r", "c", "f"}
    path = os.path.join(HERE, "lvis_v0_5_categories.json")
    with open(path, "w") as f:
        json.dump({"dataset": "lvis_v0.5", "counts": {k: counts[k] for k in "rcf"}, "categories": rows}, f, indent=0)
        f.write("\n")
    print("lvis_v0_5_categories %.1f KiB; r / c / f" % (os.path.getsize(path) / 1024), [counts[k] for k in "rcf"])


if __name__ == "__main__":
    main()
