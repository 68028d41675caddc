#!/usr/bin/env python3
"""Adds the Murcko scaffold columns a scaffold model's loader reads (src_scaffold / trg_scaffold, laid out as the
reference's preprocess.py lays them out: each behind its `src` / `trg` column) to a CSV that has only SMILES, without
rdkit: scaffold.SmilesScaffolds over the file's own tokens, --chunk rows per launch -- scaffold_rows on a GPU,
scaffold_reference (the host statement) on the CPU.  A row without a scaffold (acyclic, a stereo mark, a dot, bad syntax,
longer than 255 tokens) gets an empty string; the status counts are printed.

    tools/add_scaffolds.py in.csv out.csv [--smiles-col src] [--trg-col trg] [--chunk 65536] [--device cuda|cpu]

What the scaffolds are and where they differ from rdkit's: gct_plus_amd/scaffold.py."""
import argparse
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gct_plus_amd import ops  # noqa: E402
from gct_plus_amd.data import tokenize  # noqa: E402
from gct_plus_amd.scaffold import SmilesScaffolds  # noqa: E402

STATUS_NAMES = {getattr(ops, n): n[4:] for n in ("SCA_OK", "SCA_ACYCLIC", "SCA_SYNTAX", "SCA_UNSUPPORTED", "SCA_NO_TOKEN",
                                                 "SCA_NO_RING", "SCA_TOO_LONG")}
STATUS_NAMES[-1] = "NO_SPAN"
SPECIALS = ["<pad>", "<eos>", "(", ")", "[nH]"] + [str(k) for k in range(1, 10)] + [f"%{k}" for k in range(10, 64)]


def vocabulary(smiles):
    """The tokens of the strings behind what a spelling may need beside them: parentheses, ring numbers and [nH]."""
    seen = {t for s in smiles for t in tokenize(s)}
    return SPECIALS + sorted(seen - set(SPECIALS))


def scaffold_column(smiles, chunk=65536, device="cpu"):
    """(scaffold strings, Counter of status names) of a list of SMILES strings, `chunk` rows per launch."""
    smiles = [str(s) for s in smiles]
    if int(chunk) < 1:
        raise ValueError(f"chunk must be at least 1, got {chunk}")
    vocab = vocabulary(smiles)
    stoi = {t: i for i, t in enumerate(vocab)}
    sc = SmilesScaffolds(vocab, 0, 1)
    out, counts = [], collections.Counter()
    for lo in range(0, len(smiles), int(chunk)):
        ids = [[stoi[t] for t in tokenize(s)] + [1] for s in smiles[lo:lo + int(chunk)]]
        W = min(max(len(r) for r in ids), ops.SCA_MAX_SPAN)
        ys = torch.tensor([(r + [0] * (W - len(r)))[:W] for r in ids], dtype=torch.int64)   # (a longer row loses its <eos>)
        start = torch.zeros(len(ids), dtype=torch.int64)
        width = min(W + 32, ops.SCA_MAX_SPAN)
        if torch.device(device).type == "cuda":
            got = sc.scaffold_rows(ys.to(device), start, out_width=width)
        else:
            got = sc.scaffold_reference(ys, start, out_width=width)
        for row, n, st in zip(got.tokens.cpu().tolist(), got.info[:, 3].cpu().tolist(), got.info[:, 0].cpu().tolist()):
            out.append("".join(vocab[t] for t in row[:n]))
            counts[STATUS_NAMES[st]] += 1
    return out, counts


def add_columns(frame, smiles_col="src", trg_col="trg", chunk=65536, device="cpu"):
    """A copy of the pandas frame with src_scaffold behind `smiles_col` and trg_scaffold behind `trg_col` (when the frame
    has one; both hold the scaffold of their own column), and the status counts of the source column."""
    if smiles_col not in frame.columns:
        raise ValueError(f"no column {smiles_col!r} among {list(frame.columns)}")
    frame = frame.drop(columns=[c for c in ("src_scaffold", "trg_scaffold") if c in frame.columns])
    src, counts = scaffold_column(frame[smiles_col].tolist(), chunk, device)
    frame.insert(list(frame.columns).index(smiles_col) + 1, "src_scaffold", src)
    if trg_col in frame.columns:
        same = frame[trg_col].astype(str).tolist() == frame[smiles_col].astype(str).tolist()
        trg = src if same else scaffold_column(frame[trg_col].tolist(), chunk, device)[0]
        frame.insert(list(frame.columns).index(trg_col) + 1, "trg_scaffold", trg)
    return frame, counts


def main(argv=None):
    import pandas as pd
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("input"), ap.add_argument("output")
    ap.add_argument("--smiles-col", default="src")
    ap.add_argument("--trg-col", default="trg")
    ap.add_argument("--chunk", type=int, default=65536, help="rows per launch")
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    a = ap.parse_args(argv)
    frame, counts = add_columns(pd.read_csv(a.input), a.smiles_col, a.trg_col, a.chunk, a.device)
    frame.to_csv(a.output, index=False)
    print(f"add_scaffolds: {len(frame)} rows on {a.device}; " + ", ".join(f"{k} {v}" for k, v in sorted(counts.items())))


if __name__ == "__main__":
    main()
