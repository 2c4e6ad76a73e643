"""Expected strings of the grounding tail's host side (ziragroundingdino_amd/grounding.py) from the reference's own functions:
``get_phrases_from_posmap(posmap, tokenized, caption).replace(".", "")`` (groundingdino/util/utils.py:598-624, as
``predict`` calls it, util/inference.py:73-77) and ``preprocess_caption`` (util/inference.py:17-21).  The tokenization is a
stand-in that only has the ``token_to_word`` table the function reads.  Data only: captions, tables, masks, strings.
    python tests/golden/gen_grounding_golden.py      (needs /root/reference; never runs on the GPU box)
"""
import ast
import contextlib
import importlib
import io
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

T = 256


class Tokenized:
    def __init__(self, table):
        self.table = table

    def token_to_word(self, i):
        return self.table[i] if i < len(self.table) else None


def reference_preprocess_caption():
    """util/inference.py imports OpenCV and supervision at its top; the one function is taken out of its syntax tree."""
    path = os.path.join(ref_import.REF, "groundingdino", "util", "inference.py")
    with open(path) as fh:
        tree = ast.parse(fh.read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "preprocess_caption"]
    scope = {}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), scope)
    return scope["preprocess_caption"]


def words_of(tokens):
    words = [0] * (T // 32)
    for t in tokens:
        words[t // 32] |= 1 << (t % 32)
    return words


def main():
    ref_import.load()
    get_phrases = importlib.import_module("groundingdino.util.utils").get_phrases_from_posmap
    preprocess = reference_preprocess_caption()

    long_caption = ".".join("w%d" % i for i in range(255)) + "."
    # (name, caption, token_to_word table, set tokens)
    specs = [
        ("special tokens only", "cat . dog .", [None, 0, 1, 2, 3, None], [0, 5]),
        ("nothing set", "cat . dog .", [None, 0, 1, 2, 3, None], []),
        ("one word", "cat . dog .", [None, 0, 1, 2, 3, None], [1]),
        ("one word and a special token", "cat . dog .", [None, 0, 1, 2, 3, None], [0, 2]),
        ("words of two categories", "cat . dog . crab .", [None, 0, 1, 2, 3, 4, 5, None], [1, 2, 3]),
        ("padding behind the end", "cat . dog .", [None, 0, 1, 2, 3, None, None, None], [2, 6, 7, 200]),
        ("a word in several tokens, all set", "jellyfish.puffin.", [None, 0, 0, 0, 1, 1, 1, None], [1, 2, 3]),
        ("a word in several tokens, the last set", "jellyfish.puffin.", [None, 0, 0, 0, 1, 1, 1, None], [3, 6]),
        ("the same word twice", "jellyfish.puffin.", [None, 0, 0, 0, 1, 1, 1, None], [4, 5]),
        ("token 255", long_caption, [None] + list(range(255)), [255]),
        ("tokens 1, 31, 32, 224 and 255", long_caption, [None] + list(range(255)), [1, 31, 32, 224, 255]),
        ("every token", long_caption, [None] + list(range(255)), list(range(T))),
    ]
    cases = []
    for name, caption, table, tokens in specs:
        posmap = torch.zeros(T, dtype=torch.bool)
        posmap[torch.tensor(tokens, dtype=torch.long)] = True
        with contextlib.redirect_stdout(io.StringIO()):           # (the function prints its word lists)
            phrase = get_phrases(posmap, Tokenized(table), caption).replace(".", "")
        cases.append({"name": name, "caption": caption, "token_to_word": table, "tokens": tokens,
                      "token_bits": words_of(tokens), "phrase": phrase})
    raw = ["  A Cat. ", "dog", "Fish . Crab .", "", "RED CAR . blue bus", "\tturtle .\n"]
    out = {"phrases": cases, "captions": [{"raw": r, "preprocessed": preprocess(r)} for r in raw]}
    path = os.path.join(HERE, "grounding_phrases.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=0, sort_keys=True)
    print("wrote", path, len(cases), "phrase cases,", len(raw), "captions, %.1f KB" % (os.path.getsize(path) / 1e3))
    for c in cases:
        print("  %-40s %r" % (c["name"], c["phrase"][:60]))


if __name__ == "__main__":
    main()
