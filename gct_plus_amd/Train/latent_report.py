"""Which latent dimensions carry anything: per-dimension KL, moments of the posterior and active units (Burda et al.
2016) over a data loader.  Encoder forwards only, in eval() mode under no_grad; each batch adds its live latent rows
into one fp64 state on the device (ops.latent_moments: two launches) and the state is read back once, at the end."""
from typing import NamedTuple

import pandas as pd
import torch

from .. import engine, ops
from ..Model.forward_propagation1 import forward_propagation, latent_live_rows

ACTIVE_UNIT_THRESHOLD = 0.01          # Burda et al.: a unit is active when Var_x(E_q[z_j | x]) > 0.01


class LatentReport(NamedTuple):
    """Per dimension (fp64 [D] each): kl = KL per molecule, mu_mean and mu_var = mean and pooled (population) variance
    of mu over the live rows, post_var = mean posterior variance exp(log_var).  Totals: molecules, rows (live latent
    rows), active_units = #{j : mu_var_j > threshold}, kl_per_molecule = sum_j kl_j, under_floor = #{j : kl_j <=
    free_bits} (the dimensions a free-bits floor of that size would hold)."""
    kl: torch.Tensor
    mu_mean: torch.Tensor
    mu_var: torch.Tensor
    post_var: torch.Tensor
    molecules: int
    rows: int
    threshold: float
    free_bits: float
    active_units: int
    kl_per_molecule: float
    under_floor: int

    @classmethod
    def from_state(cls, acc, molecules, free_bits=0.0, threshold=ACTIVE_UNIT_THRESHOLD):
        """acc: the fp64 [6, D] state of ops.latent_moments (rows: sum mu, sum mu^2, sum exp(lv), sum lv, sum KL term,
        live rows), on any device; molecules: how many molecules it covers."""
        acc = torch.as_tensor(acc, dtype=torch.float64).cpu()
        if acc.dim() != 2 or acc.shape[0] != 6:
            raise ValueError(f"LatentReport: expected a [6, D] state, got {tuple(acc.shape)}")
        free_bits, _ = engine.check_kl_controls(free_bits)
        rows, n = int(acc[5, 0]), max(int(molecules), 1)
        r = max(rows, 1)
        mean = acc[0] / r
        var = (acc[1] / r - mean * mean).clamp_min(0.0)
        kl = acc[4] / n
        return cls(kl=kl, mu_mean=mean, mu_var=var, post_var=acc[2] / r, molecules=int(molecules), rows=rows,
                   threshold=float(threshold), free_bits=free_bits, active_units=int((var > threshold).sum()),
                   kl_per_molecule=float(kl.sum()), under_floor=int((kl <= free_bits).sum()))

    def line(self, epoch=None):
        head = 'LATENT' if epoch is None else f'LATENT(epoch {epoch})'
        return (f'{head}\tactive units: {self.active_units}/{self.kl.numel()} (Var mu > {self.threshold:g})\t'
                f'KL/molecule: {self.kl_per_molecule:.5f}\tdims with KL <= {self.free_bits:g}: {self.under_floor}\t'
                f'molecules: {self.molecules}\tlatent rows: {self.rows}')

    def to_frame(self):
        return pd.DataFrame({'KL': self.kl.tolist(), 'MU_MEAN': self.mu_mean.tolist(), 'MU_VAR': self.mu_var.tolist(),
                             'POST_VAR': self.post_var.tolist(),
                             'ACTIVE': [int(v > self.threshold) for v in self.mu_var.tolist()]})


def latent_report(args, model, dataloader, max_batches=None, threshold=ACTIVE_UNIT_THRESHOLD):
    """LatentReport of `model` (or the module a data-parallel wrapper holds) over `dataloader`'s batches, at most
    max_batches of them.  Padded source positions never count: the live rows are the encoder's key mask.  The model's
    train/eval mode is restored."""
    inner = getattr(model, 'module', model)
    conditioned = forward_propagation[args.model_type] is forward_propagation['pvaetf']
    was_training = inner.training
    inner.eval()
    acc, molecules = None, 0
    try:
        with torch.no_grad():
            for i, batch in enumerate(dataloader):
                if max_batches is not None and i >= max_batches:
                    break
                live = latent_live_rows(args.model_type, batch, args.pad_id)
                _, mu, log_var = inner.encode(batch['src'], live, batch['econds'] if conditioned else None)[:3]
                if acc is None:
                    acc = ops.latent_moments_state(mu.shape[-1], mu.device)
                ops.latent_moments(mu.float().contiguous(), log_var.float().contiguous(), live, acc)
                molecules += batch['src'].size(0)
    finally:
        inner.train(was_training)
    if acc is None:
        raise ValueError('latent_report: the data loader gave no batch')
    return LatentReport.from_state(acc, molecules, getattr(args, 'kl_free_bits', 0.0), threshold)
