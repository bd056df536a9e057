"""Golden vectors for the L2P prompt pool (MQ/libs/cl_methods/prompt.py:47-117) from the IMPORTED REFERENCE (this container
only): the reference's Prompt module on the CPU in fp32, fixed seeds -- inputs, parameters, every entry of the result
dictionary and the gradients of prompt, prompt_key and x_embed under the loss prompted.square().sum() - 0.1 * reduce_sim.
Run:  python tests/golden/make_golden_prompt.py  ->  tests/golden/prompt_pool.npz   (data only)

Cases: the fixed per-task window, top-k per row, top-k with the batch vote; all four embedding keys ('cls' with and
without cls_features).  C = 96 keeps the file small; the arithmetic does not depend on the width.

Only DECIDED draws are recorded (checked in the fp64 restatement, tests/prompt_restatement.py, and asserted here):
  * every gap between consecutive similarities among a row's k + 1 largest is above 1e-4 (the cut and the order inside it);
  * with the vote, the k-th and the (k+1)-th largest counts differ.
torch.topk leaves the order among EQUAL counts undefined; equal counts inside the cut do not change the chosen set, but
they do change the order the prompts are prepended in.  A draw on which the reference's order differs from the counting
rank (equal counts by smaller id) is redrawn as well, so the recorded indices are the restatement's exactly.  The text
rows share a common direction so that the rows of a batch mostly agree and the vote is decided after a few draws."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_import  # noqa: E402
import prompt_restatement as R  # noqa: E402

C, P, LEN, K = 96, 10, 5, 4
GAP = 1e-4
# name -> (embedding_key, mode, B, L, cls_features given)
CASES = {
    'window_mean': ('mean', 'window', 2, 7, False),
    'window_max': ('max', 'window', 2, 7, False),
    'topk_mean': ('mean', 'topk', 3, 7, False),
    'topk_mean_max': ('mean_max', 'topk', 3, 6, False),
    'topk_cls_nofeat': ('cls', 'topk', 2, 5, False),
    'vote_mean': ('mean', 'vote', 3, 7, False),
    'vote_max': ('max', 'vote', 3, 7, False),
    'vote_cls': ('cls', 'vote', 3, 4, True),
}


def decided(sim, k, vote):
    for row in sim:
        s = np.sort(row)[::-1][:k + 1]
        if np.min(s[:-1] - s[1:]) <= GAP:
            return False
    if vote:
        idx = np.stack([R.top_by_rank(r, k) for r in sim])
        counts = np.sort(np.bincount(idx.reshape(-1), minlength=sim.shape[1]))[::-1]
        if counts[k - 1] == counts[k]:
            return False
    return True


def draw(seed, B, L, with_cls):
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(1, 1, C, generator=g)
    x = base + 0.6 * torch.randn(B, L, C, generator=g)
    cls = (base[0] + 0.6 * torch.randn(B, C, generator=g)) if with_cls else None
    return x, cls


def main():
    ref_import.setup(extra_xlnet=())
    from libs.cl_methods.prompt import Prompt
    out, redraws = {}, {}
    for ci, (name, (ekey, mode, B, L, with_cls)) in enumerate(CASES.items()):
        torch.manual_seed(100 + ci)
        mod = Prompt(length=LEN, embed_dim=C, embedding_key=ekey, prompt_init='uniform', prompt_pool=True, prompt_key=True,
                     pool_size=P, top_k=K, batchwise_prompt=(mode == 'vote'), prompt_key_init='uniform')
        window = torch.arange(K, 2 * K).unsqueeze(0).expand(B, -1) if mode == 'window' else None
        for attempt in range(2000):
            seed = 1000 * (ci + 1) + attempt
            x, cls = draw(seed, B, L, with_cls)
            want = R.forward(x.numpy(), mod.prompt.detach().numpy(), mod.prompt_key.detach().numpy(),
                             idx=None if window is None else window.numpy(), k=K, batchwise=(mode == 'vote'),
                             embedding_key=ekey, cls_features=None if cls is None else cls.numpy())
            if window is None and not decided(want['similarity'], K, mode == 'vote'):
                continue
            mod.zero_grad()
            xg = x.clone().requires_grad_(True)
            res = mod(xg, prompt_mask=window, cls_features=cls)
            if not np.array_equal(res['prompt_idx'].numpy(), want['prompt_idx']):
                assert mode == 'vote', (name, seed)         # only the order among equal counts inside the cut is open
                assert sorted(res['prompt_idx'][0].tolist()) == sorted(want['prompt_idx'][0].tolist()), (name, seed)
                continue
            break
        else:
            raise RuntimeError("no decided draw for " + name)
        if window is None:
            assert decided(want['similarity'], K, mode == 'vote')
        redraws[name] = attempt
        (res['prompted_embedding'].square().sum() - 0.1 * res['reduce_sim']).backward()
        rec = {'x': x, 'prompt': mod.prompt.detach(), 'key': mod.prompt_key.detach(),
               'd_prompt': mod.prompt.grad, 'd_key': mod.prompt_key.grad, 'd_x': xg.grad,
               'total_prompt_len': torch.tensor(res['total_prompt_len'])}
        if cls is not None:
            rec['cls'] = cls
        if window is not None:
            rec['window'] = window
        for k_ in ('prompt_idx', 'prompt_norm', 'x_embed_norm', 'similarity', 'selected_key', 'reduce_sim', 'prompted_embedding'):
            rec[k_] = res[k_].detach()
        for k_, v in rec.items():
            out['%s/%s' % (name, k_)] = v.contiguous().numpy()
        print(name, 'seed', seed, 'idx', res['prompt_idx'].tolist(), 'reduce_sim %.6f' % float(res['reduce_sim']))
    out['undecided_share'] = np.array(0.0)
    path = os.path.join(HERE, 'prompt_pool.npz')
    np.savez(path, **out)
    print('redraws', redraws, '%.1f KB' % (os.path.getsize(path) / 1e3))


if __name__ == "__main__":
    main()
