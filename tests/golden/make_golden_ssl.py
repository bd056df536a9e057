"""Golden vectors for the narration-SSL branch, from the IMPORTED REFERENCE: three consecutive steps
through the reference's own MemoryBank (meta_archs.py:38-60), its unbound PtTransformer.masked_contrastive_loss (:1351-1372)
and the pooling block of its forward (:794-811), which is cut out of the imported function's source at run time and executed
as it stands -- nothing of it is restated here.  Masks [1,0,1], [0,0,0], [1,1,1] against a bank of 4 rows: the second update
wraps; the all-zero step is skipped, as the reference's `if ... .sum() > 0` does (:939).  `.cuda()` is a no-op (no GPU here).
Run:  python tests/golden/make_golden_ssl.py  ->  tests/golden/ssl_step.npz   (data only)"""
import inspect
import os
import sys
import textwrap
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

B, D, M, CN, NTOK, TS = 3, 8, 4, 6, 5, (8, 4)
MASKS = ([1, 0, 1], [0, 0, 0], [1, 1, 1])
TOK_LENS = ([5, 0, 1], [2, 5, 4], [4, 2, 5])
FEAT_LENS = ([[8, 4], [5, 3], [1, 1]], [[8, 4], [8, 4], [3, 2]], [[6, 3], [2, 1], [8, 4]])


def pooling_block(fn):
    """the statements of `forward` from `if self.training and self.narration_ssl:` to the normalisation of video_feats"""
    lines = inspect.getsource(fn).splitlines()
    first = next(i for i, l in enumerate(lines) if l.strip().startswith("if self.training and self.narration_ssl"))
    last = next(i for i in range(first, len(lines)) if lines[i].strip().startswith("video_feats = F.normalize("))
    return compile(textwrap.dedent("\n".join(lines[first:last + 1])), "<reference forward: narration pooling>", "exec")


def main():
    ref_import.setup(extra_xlnet=((32, 4),))
    import libs.modeling.meta_archs as ref
    torch.Tensor.cuda = lambda self, *a, **k: self
    block = pooling_block(ref.PtTransformer.forward)
    g = torch.Generator().manual_seed(23)
    enc = torch.nn.Linear(CN, D)
    with torch.no_grad():
        enc.weight.copy_(0.5 * torch.randn(D, CN, generator=g))
        enc.bias.copy_(0.1 * torch.randn(D, generator=g))
    bank = ref.MemoryBank(M, D)
    bank.memory = torch.randn(M, D, generator=g)
    stub = types.SimpleNamespace(training=True, narration_ssl=True, narration_encoder=enc, memory_bank=bank)
    out = {'enc_w': enc.weight.detach().numpy().copy(), 'enc_b': enc.bias.detach().numpy().copy(),
           'bank0': bank.memory.numpy().copy(), 'masks': np.array(MASKS, dtype=np.float32),
           'tok_lens': np.array(TOK_LENS, dtype=np.int32), 'feat_lens': np.array(FEAT_LENS, dtype=np.int32),
           'skipped': np.zeros(len(MASKS), dtype=np.bool_)}
    for s, (mask, tl, fl) in enumerate(zip(MASKS, TOK_LENS, FEAT_LENS)):
        tokens = torch.randn(B, CN, NTOK, generator=g).requires_grad_(True)
        feats = [(0.3 + torch.randn(B, D, T, generator=g)).requires_grad_(True) for T in TS]        # channel-first, as the reference
        m1 = (torch.arange(NTOK)[None, :] < torch.tensor(tl)[:, None]).unsqueeze(1)
        fmasks = [(torch.arange(T)[None, :] < torch.tensor([r[l] for r in fl])[:, None]).unsqueeze(1) for l, T in enumerate(TS)]
        m0 = torch.tensor(mask, dtype=torch.float32)
        ns = dict(self=stub, src_narration=tokens, src_narration_mask=(m0, m1), fpn_feats=feats, fpn_masks=fmasks, torch=torch,
                  F=torch.nn.functional)
        exec(block, ns)
        narration_feats, video_feats = ns['narration_feats'], ns['video_feats']
        out['tokens%d' % s] = tokens.detach().numpy().copy()
        for l, f in enumerate(feats):
            out['feats%d_%d' % (s, l)] = f.detach().permute(0, 2, 1).contiguous().numpy().copy()     # token-major [B, T, C]
        if m0.sum() > 0:                                                                          # (:939-945)
            mb = m0.to(torch.bool)
            bank.update(narration_feats[mb])
            loss = ref.PtTransformer.masked_contrastive_loss(stub, narration_feats, video_feats, mb)
            enc.zero_grad()
            loss.backward()
            out['loss%d' % s] = np.float64(loss.item())
            out['d_tokens%d' % s] = tokens.grad.numpy().copy()
            for l, f in enumerate(feats):
                out['d_feats%d_%d' % (s, l)] = f.grad.permute(0, 2, 1).contiguous().numpy().copy()
            out['d_enc_w%d' % s], out['d_enc_b%d' % s] = enc.weight.grad.numpy().copy(), enc.bias.grad.numpy().copy()
        else:
            out['skipped'][s] = True
        out['bank%d' % s] = bank.memory.detach().numpy().copy()
        out['ptr%d' % s] = np.int64(bank.ptr)
    np.savez(os.path.join(HERE, 'ssl_step.npz'), **out)
    print({k: (v.shape if hasattr(v, 'shape') and v.shape else v) for k, v in out.items() if k.startswith(('loss', 'ptr', 'skipped'))})


if __name__ == "__main__":
    main()
