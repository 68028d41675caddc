#!/usr/bin/env python3
"""Policy-gradient fine-tuning end to end on a synthetic-weight pscavaetf (tiny by default, --full: d512 / 6 layers):
--rounds times  sample --n molecules (multinomial, one scaffold) -> reward -> Train/finetune.reinforce_step.
The reward is smiles.SmilesGrammar.well_formed of the generated tokens (1 or 0), so no chemistry toolkit is needed: a
randomly initialised model seldom closes its rings and branches and ends with <eos>, and the update teaches it to.
Prints the well-formed rate of a fixed evaluation batch before and after -- with the number of DISTINCT strings in it and
the policy's mean entropy per token, which show the collapse a reward alone ends in --, the rate of every round, and the
time of a reinforce_step (forward + backward + optimizer, the sampling not included).
--entropy-coef / --kl-coef: the regularised step (an entropy bonus; a KL penalty against Train/finetune.frozen_prior of
the starting weights, which costs a second, forward-only decoder pass).  No coefficient is prescribed.
--ppo-epochs K [--clip E]: Train/finetune.ppo_update instead -- K updates per sampled batch under PPO's clipped surrogate
against the log-probabilities the batch was sampled with (one more forward-only pass per batch); the printed time is
that of the whole update, and per epoch.
--max-grad-norm C: every update's gradient is clipped to the global L2 norm C on the device (FusedAdam's max_grad_norm,
through the max_grad_norm argument of the two functions); the rounds then also print the pre-clip norm.  No value is
prescribed.

--reward chemistry: the sampler decodes with well_formed=True (every row is syntactically right already) and the reward is
Train/finetune.validity_reward of Sampling.check_rows -- smiles.SmilesChemistry's valence / ring-bond / aromaticity check,
one launch on the device instead of the Python loop over the rows; the printed rate is then the VALID share.  The default,
--reward grammar, is the run described above and prints what it always did.

--reward NAME:T:TOL (NAME a descriptor.DescRows column: tpsa, mw, hbd, hba, rotatable, rings, ...): constrained decoding
as under --reward chemistry, and the reward is validity_reward x Train/finetune.property_reward(Sampling.descriptors(rows),
NAME, T, TOL) = max(0, 1 - |value - T| / TOL) -- the policy is paid for valid molecules near the property target; the
printed rate is then the MEAN REWARD.

--report-descriptors: one more line at the end: the means of mw, tpsa, hbd, hba, rotatable and rings over the rows of the
evaluation batch that have descriptors (descriptor.SmilesDescriptors, on the device), before and after.

--report-unique: one more line at the end: the DISTINCT MOLECULES of the evaluation batch before and after, beside the
distinct strings -- Sampling.molecule_keys and molkey.first_occurrence, on the device: a policy that writes one molecule
in five spellings counts once.

--report-diversity: one more line at the end: the INTERNAL DIVERSITY (moses' intDiv: 1 - the mean Tanimoto similarity of
all pairs, self pairs included) of the rows of the evaluation batch that have a fingerprint, before and after --
Sampling.fingerprints and fingerprint.internal_diversity, on the device: a collapsed policy falls towards 0.

--report-scaffold: one more line at the end: same_scaffold of the evaluation batch before and after -- the share of its
chemically valid rows whose molecule has the Murcko scaffold the row was given (Sampling.scaffold_report and
molkey.scaffold_metrics, on the device; Train/finetune.scaffold_reward is the same verdict as a reward).

--time-step: no sampling; --n fixed rows of MOSES-like lengths (clip(round(N(35, 8)), 15, 78) tokens + <eos> behind a
scaffold prefix), --rounds reinforce_steps on them after two warm-up steps: the figure to put next to a bench.py
training step of the same batch size (recorded in DESIGN 4, not gated).  With --ppo-epochs it times ONE epoch:
ppo_update(epochs=1) against a sampling-time table taken once, before the first step, and that pass on its own."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--full", action="store_true", help="the full-size model (N 6, d_model 512, dff 2048, h 8, latent 128)")
ap.add_argument("--n", type=int, default=512, help="molecules per round")
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--lr", type=float, default=1e-4)
ap.add_argument("--max-strlen", type=int, default=40)
ap.add_argument("--scaffold", default="c1ccccc1")
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--entropy-coef", type=float, default=0.0, help="entropy bonus per scored token (reinforce_step)")
ap.add_argument("--kl-coef", type=float, default=0.0,
                help="penalty on KL(policy || frozen starting weights) per scored token")
ap.add_argument("--ppo-epochs", type=int, default=0,
                help="K > 0: ppo_update with K epochs per sampled batch instead of one reinforce_step")
ap.add_argument("--clip", type=float, default=0.2, help="PPO's clip: ratios are held in [1 - E, 1 + E]")
ap.add_argument("--max-grad-norm", type=float, default=None,
                help="bound on the global L2 norm of every update's gradient (FusedAdam clips on the device)")
def reward_kind(text):
    """grammar, chemistry, or NAME:T:TOL -> (NAME, T, TOL)."""
    if text in ("grammar", "chemistry"):
        return text
    parts = text.split(":")
    try:
        name, target, tol = parts[0], float(parts[1]), float(parts[2])
        if len(parts) != 3 or not tol > 0.0:
            raise ValueError
    except (IndexError, ValueError):
        raise argparse.ArgumentTypeError(f"`{text}`: grammar, chemistry or NAME:T:TOL with TOL > 0, such as tpsa:40:20")
    return name, target, tol


ap.add_argument("--reward", type=reward_kind, default="grammar",
                help="grammar: 1 for a well-formed string; chemistry: constrained decoding, 1 for a chemically valid one; "
                     "NAME:T:TOL: constrained decoding, validity x max(0, 1 - |descriptor NAME - T| / TOL)")
ap.add_argument("--report-descriptors", action="store_true",
                help="one more line at the end: mean mw, tpsa, hbd, hba, rotatable, rings of the evaluation batch")
ap.add_argument("--report-valid", action="store_true",
                help="one more line at the end: the chemically valid share of the evaluation batch before and after")
ap.add_argument("--report-unique", action="store_true",
                help="one more line at the end: distinct molecules (molecule keys) beside the distinct strings")
ap.add_argument("--report-diversity", action="store_true",
                help="one more line at the end: the internal diversity (intDiv) of the evaluation batch before and after")
ap.add_argument("--report-scaffold", action="store_true",
                help="one more line at the end: the share of valid rows that have the scaffold they were given")
ap.add_argument("--time-step", action="store_true",
                help="time reinforce_step (one ppo_update epoch with --ppo-epochs) on fixed rows of MOSES-like lengths")
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gct_plus_amd import data, synthetic  # noqa: E402
from gct_plus_amd.smiles import SmilesGrammar  # noqa: E402
from gct_plus_amd.fingerprint import internal_diversity  # noqa: E402
from gct_plus_amd.Inference.sampling_tool import DecodedRows, PscavaetfSampling  # noqa: E402
from gct_plus_amd.Model import model_dict  # noqa: E402
from gct_plus_amd.molkey import first_occurrence, scaffold_metrics  # noqa: E402
from gct_plus_amd.optim import FusedAdam  # noqa: E402
from gct_plus_amd.Train.finetune import (frozen_prior, ppo_update, property_reward, reinforce_step,  # noqa: E402
                                         validity_reward)

mtype = "pscavaetf"
nc = synthetic.n_conds(mtype)
dims = (dict(N=6, d_model=512, dff=2048, h=8, latent_dim=128) if a.full
        else dict(N=2, d_model=64, dff=128, h=4, latent_dim=16))
TRG = data.Vocab(synthetic.GRAMMAR_VOCAB)
SRC = data.Vocab([t for t in synthetic.GRAMMAR_VOCAB if t not in ("<sos>", "<eos>")])
torch.manual_seed(a.seed)
model = model_dict[mtype](len(SRC), len(TRG), dropout=0.0, nconds=nc, use_cond2lat=True, **dims).cuda()
sampler = PscavaetfSampling(model, SRC, TRG, latent_dim=dims["latent_dim"], max_strlen=a.max_strlen, cond_dim=nc,
                            decode_algo="multinomial", seed=a.seed, well_formed=a.reward != "grammar")
PROPERTY = a.reward if isinstance(a.reward, tuple) else None
WHAT = "valid" if a.reward == "chemistry" else f"reward({PROPERTY[0]})" if PROPERTY else "well-formed"
if PROPERTY:
    sampler.descriptors(["C"]).column(PROPERTY[0])             # (an unknown column name ends the run here)
grammar = SmilesGrammar(TRG.itos, sampler.pad_id, sampler.eos_id) if a.reward == "grammar" else None
opt = FusedAdam(model.parameters(), lr=a.lr, betas=(0.9, 0.98), eps=1e-9, model=model)
gen = torch.Generator().manual_seed(a.seed)
prior = frozen_prior(model) if a.kl_coef else None


def timed_step(rows, reward, **ppo):
    """One update, timed: reinforce_step, or with --ppo-epochs ppo_update (its list of per-epoch results)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if a.ppo_epochs:
        stats = ppo_update(sampler, opt, rows, reward, **dict(dict(epochs=a.ppo_epochs), **ppo), clip=a.clip,
                           entropy_coef=a.entropy_coef, kl_coef=a.kl_coef, prior=prior, max_grad_norm=a.max_grad_norm)
    else:
        stats = reinforce_step(sampler, opt, rows, reward, entropy_coef=a.entropy_coef, kl_coef=a.kl_coef, prior=prior,
                               max_grad_norm=a.max_grad_norm)
    torch.cuda.synchronize()
    return stats, (time.perf_counter() - t0) * 1e3


if a.time_step:
    n, Le = a.n, 80 + nc
    sca = sampler.smi_to_id(a.scaffold)
    t0 = len(sca) + 2
    ln = np.clip(np.rint(np.random.default_rng(0).normal(35, 8, n)), 15, 78).astype(np.int64)
    W = t0 + int(ln.max()) + 1
    ys = torch.randint(5, len(TRG), (n, W), generator=gen)
    ys[:, :t0] = torch.tensor([sampler.sos_id] + sca + [sampler.sep_id])
    cols, end = torch.arange(W)[None, :], torch.from_numpy(ln)[:, None] + t0
    ys[cols == end] = sampler.eos_id
    ys[cols > end] = sampler.pad_id
    src_mask = (torch.arange(Le)[None, :] < (torch.from_numpy(ln) + t0 - 1 + nc)[:, None]).unsqueeze(1)
    rows = DecodedRows(torch.randn(n, Le, dims["latent_dim"], generator=gen).cuda(), ys.cuda(), src_mask.cuda(),
                       torch.randn(n, nc, generator=gen).cuda(), torch.full((n,), t0))
    reward = torch.rand(n, generator=gen)
    if a.ppo_epochs:
        model.eval()
        old_ms = []
        for _ in range(5):                                # the forward-only pass a batch pays once
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            with torch.no_grad():
                old = sampler.logp(*rows).token_logp
            torch.cuda.synchronize()
            old_ms.append((time.perf_counter() - t1) * 1e3)
        for _ in range(2):
            timed_step(rows, reward, epochs=1, old_token_logp=old)
        ms = []
        for i in range(a.rounds):
            (stats,), dt = timed_step(rows, reward, epochs=1, old_token_logp=old)
            ms.append(dt)
            print(f"epoch {i}: {dt:8.2f} ms  loss {stats['loss']:.4f}  clipped {stats['clip_fraction']:.3f}  approx_kl "
                  f"{stats['approx_kl']:.5f}  tokens {stats['tokens']}", flush=True)
        print(f"ppo_update epoch on {n} {'full-size' if a.full else 'tiny'} {mtype} rows of {W} columns ({stats['tokens']} "
              f"scored tokens), clip {a.clip}: median {float(np.median(ms)):.2f} ms, best {min(ms):.2f} ms of {len(ms)}; "
              f"the sampling-time table (one forward-only pass per batch): median {float(np.median(old_ms[1:])):.2f} ms")
        sys.exit(0)
    for _ in range(2):
        timed_step(rows, reward)
    ms = []
    for i in range(a.rounds):
        stats, dt = timed_step(rows, reward)
        ms.append(dt)
        print(f"step {i}: {dt:8.2f} ms  loss {stats['loss']:.4f}  tokens {stats['tokens']}", flush=True)
    print(f"reinforce_step on {n} {'full-size' if a.full else 'tiny'} {mtype} rows of {W} columns ({stats['tokens']} scored "
          f"tokens): median {float(np.median(ms)):.2f} ms, best {min(ms):.2f} ms of {len(ms)}")
    sys.exit(0)


def sample(n, seed):
    """n molecules of one scaffold -> (DecodedRows, reward [n]: 1 where the generated tokens are a well-formed string)."""
    sampler.seed = seed
    g = torch.Generator().manual_seed(seed)
    toklen = [a.max_strlen // 2] * n
    zs = torch.randn(n, len(sampler.smi_to_id(a.scaffold)) + 1 + toklen[0], dims["latent_dim"], generator=g)
    out = sampler.sample_smiles(torch.randn(n, nc, generator=g).numpy(), a.scaffold, zs=zs, toklen=toklen, transform=False,
                                return_rows=True)
    rows = out[-1]
    if a.reward == "chemistry":
        return rows, validity_reward(sampler.check_rows(rows))
    if PROPERTY:
        return rows, validity_reward(sampler.check_rows(rows)) * property_reward(sampler.descriptors(rows), *PROPERTY)
    t0 = int(rows.prefix_lens[0])
    reward = torch.tensor([float(grammar.well_formed(r)) for r in rows.ys[:, t0:].cpu().tolist()])
    return rows, reward


def evaluate():
    """The fixed evaluation batch under the current weights: (well-formed rate, distinct generated strings, mean entropy
    of the policy per scored token)."""
    rows, reward = sample(a.n, EVAL_SEED)
    t0 = int(rows.prefix_lens[0])
    distinct = len({tuple(t for t in r if t != sampler.pad_id) for r in rows.ys[:, t0:].cpu().tolist()})
    with torch.no_grad():
        terms = sampler.policy_terms(*rows)
    if a.report_valid:
        VALID_SHARE.append(float(validity_reward(sampler.check_rows(rows)).mean()))
    if a.report_unique:
        mk = sampler.molecule_keys(rows)
        MOLECULES.append(int(first_occurrence(mk, valid=mk.info[:, 0] >= 0).sum()))
    if a.report_diversity:
        fps = sampler.fingerprints(rows)
        DIVERSITY.append((internal_diversity(fps), int((fps.info[:, 1] > 0).sum())))
    if a.report_descriptors:
        d = sampler.descriptors(rows)
        k = d.ok.sum().clamp(min=1).to(torch.float64)
        cols = d.columns(DESCRIPTOR_COLUMNS).to(torch.float64)
        means = torch.where(d.ok[:, None], cols, torch.zeros_like(cols)).sum(0) / k
        DESCRIPTORS.append((means.tolist(), int(d.ok.sum())))
    if a.report_scaffold:
        SAME_SCAFFOLD.append(scaffold_metrics(sampler.check_rows(rows), sampler.scaffold_report(rows)))
    return float(reward.mean()), distinct, float(terms.entropy.sum() / terms.tokens.sum())


EVAL_SEED = 10 ** 6
VALID_SHARE = []
MOLECULES = []
SAME_SCAFFOLD = []
DIVERSITY = []
DESCRIPTORS = []
DESCRIPTOR_COLUMNS = ("mw", "tpsa", "hbd", "hba", "rotatable", "rings")
before = evaluate()
reg = f", entropy_coef {a.entropy_coef}, kl_coef {a.kl_coef}" if a.entropy_coef or a.kl_coef else ""
if a.ppo_epochs:
    reg += f", {a.ppo_epochs} PPO epochs per round, clip {a.clip}"
if a.max_grad_norm is not None:
    reg += f", max_grad_norm {a.max_grad_norm:g}"
print(f"{'full-size' if a.full else 'tiny'} {mtype}, {a.n} molecules per round, lr {a.lr}{reg}: evaluation batch before "
      f"fine-tuning: {WHAT} {before[0]:.3f}, {before[1]} distinct strings, entropy {before[2]:.3f} per token",
      flush=True)
ms = []
for k in range(a.rounds):
    rows, reward = sample(a.n, a.seed * 1000 + k)
    stats, dt = timed_step(rows, reward)
    ms.append(dt)
    if a.ppo_epochs:
        last = stats[-1]
        more = "".join(f"  {key[5:]} {last[key]:7.4f}" for key in ("mean_entropy", "mean_kl") if key in last)
        if "grad_norm" in last:
            more += (f"  grad norm {max(s['grad_norm'] for s in stats):8.4f}  clipped updates "
                     f"{sum(s['clipped_updates'] for s in stats)}")
        print(f"round {k:3d}: {WHAT} {float(reward.mean()):.3f}  loss {stats[0]['loss']:8.4f} -> {last['loss']:8.4f}  "
              f"clipped {last['clip_fraction']:.3f}  approx_kl {last['approx_kl']:.5f}{more}  update {dt:7.2f} ms "
              f"({dt / len(stats):.2f} per epoch)", flush=True)
        continue
    more = "".join(f"  {key[5:]} {stats[key]:7.4f}" for key in ("mean_entropy", "mean_kl") if key in stats)
    if "grad_norm" in stats:
        more += f"  grad norm {stats['grad_norm']:8.4f}{' (clipped)' if stats['clipped'] else ''}"
    print(f"round {k:3d}: {WHAT} {stats['mean_reward']:.3f}  mean logp {stats['mean_logp']:8.3f}  loss "
          f"{stats['loss']:8.4f}{more}  step {dt:7.2f} ms", flush=True)
after = evaluate()
print(f"evaluation batch of {a.n}: {WHAT} {before[0]:.3f} -> {after[0]:.3f}, distinct strings {before[1]} -> "
      f"{after[1]}, entropy per token {before[2]:.3f} -> {after[2]:.3f} after {a.rounds} rounds{reg}; "
      f"{'ppo_update' if a.ppo_epochs else 'reinforce_step'} median {float(np.median(ms[1:] or ms)):.2f} ms")
if a.report_valid:
    print(f"chemically valid share of the evaluation batch (smiles.SmilesChemistry): {VALID_SHARE[0]:.3f} -> "
          f"{VALID_SHARE[1]:.3f}")
if a.report_unique:
    print(f"distinct molecules of the evaluation batch (molkey.SmilesKeys; a row without a graph counts as its string, one without "
          f"<eos> not at all): "
          f"{MOLECULES[0]} -> {MOLECULES[1]}, beside distinct strings {before[1]} -> {after[1]}")
if a.report_diversity:
    (b, nb), (c, nc) = DIVERSITY
    print(f"internal diversity of the evaluation batch (fingerprint.SmilesFingerprints; intDiv over the rows that have a "
          f"fingerprint): {b:.4f} -> {c:.4f} ({nb} -> {nc} rows)")
if a.report_descriptors:
    (b, nb), (c, nc) = DESCRIPTORS
    print(f"mean descriptors of the evaluation batch (descriptor.SmilesDescriptors; over the rows that have them, {nb} -> "
          f"{nc}): " + ", ".join(f"{name} {x:.2f} -> {y:.2f}" for name, x, y in zip(DESCRIPTOR_COLUMNS, b, c)))
if a.report_scaffold:
    b, c = SAME_SCAFFOLD
    print(f"same_scaffold of the evaluation batch (scaffold.SmilesScaffolds; valid rows whose Murcko scaffold is {a.scaffold}): "
          f"{b['same_scaffold']:.3f} -> {c['same_scaffold']:.3f} ({b['n_same']} of {b['n_valid']} -> {c['n_same']} of "
          f"{c['n_valid']} valid rows), distinct scaffolds among them {b['n_scaffolds']} -> {c['n_scaffolds']}")
