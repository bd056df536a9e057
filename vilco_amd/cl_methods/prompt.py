"""L2P prompt pool used by the ViLCo method inside `forward` (reference:
MQ/libs/cl_methods/prompt.py:4-116): cosine similarity between the mean text token and learnable
keys, top-k (or a fixed per-task window during training) prompts of `length` tokens each are
prepended to the text sequence.  On the device the whole forward is ONE operator, ops.prompt_pool (csrc/prompt.hip: match,
batch vote and prepend in two launches, selections by counting rank, no host read; the module's batch vote keeps the
reference's order among equal counts, see _forward_fused); VILCO_FUSED_PROMPT=0 (ops.fused_prompt)
keeps the tensor-op body below for A/B runs, and CPU tensors always take it."""
import torch
import torch.nn as nn

from .. import ops


class Prompt(nn.Module):
    def __init__(self, length=5, embed_dim=768, embedding_key='mean', prompt_init='uniform', prompt_pool=False,
                 prompt_key=False, pool_size=None, top_k=None, batchwise_prompt=False, prompt_key_init='uniform'):
        super().__init__()
        self.length, self.embed_dim, self.prompt_pool = length, embed_dim, prompt_pool
        self.embedding_key, self.prompt_init = embedding_key, prompt_init
        self.pool_size, self.top_k, self.batchwise_prompt = pool_size, top_k, batchwise_prompt
        if not prompt_pool:
            raise NotImplementedError("the MQ configs only build Prompt with prompt_pool=True (meta_archs.py:643)")

        def make(shape, init):
            p = nn.Parameter(torch.zeros(shape) if init == 'zero' else torch.randn(shape))
            if init == 'uniform':
                nn.init.uniform_(p, -1, 1)
            return p
        self.prompt = make((pool_size, length, embed_dim), prompt_init)
        if prompt_key:
            self.prompt_key = make((pool_size, embed_dim), prompt_key_init)
        else:
            self.prompt_key = torch.mean(self.prompt, dim=1)

    @staticmethod
    def l2_normalize(x, dim=None, epsilon=1e-12):
        sq = torch.sum(x ** 2, dim=dim, keepdim=True)
        return x * torch.rsqrt(torch.clamp_min(sq, epsilon))       # == maximum(sq, eps): no host scalar to upload

    def forward(self, x_embed, prompt_mask=None, cls_features=None):
        if x_embed.is_cuda and ops.fused_prompt:
            return self._forward_fused(x_embed, prompt_mask, cls_features)
        return self._forward_tensor_ops(x_embed, prompt_mask, cls_features)

    def _forward_fused(self, x_embed, prompt_mask, cls_features):
        key = self.prompt_key
        if key.device != x_embed.device:                            # prompt_key=False: a plain tensor that .to() does not move
            key = self.prompt_key = key.to(x_embed.device)
        idx = None
        if prompt_mask is not None:
            idx = prompt_mask.to(device=x_embed.device, dtype=torch.int64)
        elif self.batchwise_prompt:
            # The op's own vote orders equal counts by smaller id (a counting rank).  The reference orders them as torch.topk
            # happens to on its compacted count array (prompt.py:72-82), and with the mask it then puts over the prompted text
            # (meta_archs.py:775-779: the first len(text) positions only) the ORDER decides which prompts are seen at all: at
            # B = 1, where every count is 1, the two orders give outputs 10 % apart.  So the module keeps the reference's
            # order: the rows' picks come from the op, the vote below rebuilds the array the reference hands to torch.topk
            # at its fixed size (no torch.unique: nothing is read on the host, the forward can be captured), and the op then
            # runs on the voted list as a window.
            with torch.no_grad():
                rows = ops.prompt_pool(x_embed.detach(), self.prompt.detach(), key.detach(), top_k=self.top_k, batchwise=False,
                                       embedding_key=self.embedding_key, cls_features=cls_features)[2]
                idx = self._vote(rows)
        prompted, reduce_sim, idx, sim, pn, xn, key_sel = ops.prompt_pool(
            x_embed, self.prompt, key, idx=idx, top_k=self.top_k, batchwise=self.batchwise_prompt,
            embedding_key=self.embedding_key, cls_features=cls_features)
        return {'prompt_idx': idx, 'prompt_norm': pn, 'x_embed_norm': xn, 'similarity': sim, 'selected_key': key_sel,
                'reduce_sim': reduce_sim, 'total_prompt_len': idx.shape[1] * self.length, 'prompted_embedding': prompted}

    def _vote(self, rows):
        """rows [B, k] int64 -> the voted list for every row, ties as in the tensor-op body: torch.topk over the counts of the
        ids present (ascending, compacted to the front) padded with zeros to pool_size -- the array torch.unique + cat build
        there, formed at its fixed size by a scatter"""
        P, dev = self.pool_size, rows.device
        flat = rows.reshape(-1)
        dense = torch.zeros(P, dtype=torch.int64, device=dev).scatter_add_(0, flat, torch.ones_like(flat))
        present = dense > 0
        slot = torch.where(present, torch.cumsum(present, 0) - 1, torch.full_like(dense, P))     # absent ids: a spare slot
        ids = flat.min().expand(P + 1).clone().scatter_(0, slot, torch.arange(P, device=dev))[:P]
        counts = torch.zeros(P + 1, dtype=torch.int64, device=dev).scatter_(0, slot, dense)[:P]
        _, major = torch.topk(counts, k=self.top_k)
        return ids[major].unsqueeze(0).repeat(rows.shape[0], 1)

    def _forward_tensor_ops(self, x_embed, prompt_mask=None, cls_features=None):
        if self.embedding_key == 'mean':
            x_key = torch.mean(x_embed, dim=1)
        elif self.embedding_key == 'max':
            x_key = torch.max(x_embed, dim=1)[0]
        elif self.embedding_key == 'mean_max':
            x_key = torch.max(x_embed, dim=1)[0] + 2 * torch.mean(x_embed, dim=1)
        elif self.embedding_key == 'cls':
            x_key = torch.max(x_embed, dim=1)[0] if cls_features is None else cls_features
        else:
            raise NotImplementedError("Not supported way of calculating embedding keys!")
        prompt_norm = self.l2_normalize(self.prompt_key, dim=1)
        x_norm = self.l2_normalize(x_key, dim=1)
        similarity = x_norm @ prompt_norm.t()                       # [B, pool]

        if prompt_mask is None:
            _, idx = torch.topk(similarity, k=self.top_k, dim=1)
            if self.batchwise_prompt:
                ids, counts = torch.unique(idx, return_counts=True, sorted=True)
                if ids.shape[0] < self.pool_size:
                    pad = self.pool_size - ids.shape[0]
                    ids = torch.cat([ids, torch.full((pad,), torch.min(idx.flatten()), device=ids.device)])
                    counts = torch.cat([counts, torch.full((pad,), 0, device=counts.device)])
                _, major = torch.topk(counts, k=self.top_k)
                idx = ids[major].expand(x_embed.shape[0], -1)
        else:
            idx = prompt_mask

        raw = self.prompt[idx]                                      # [B, top_k, length, C]
        B, k, length, c = raw.shape
        batched_prompt = raw.reshape(B, k * length, c)
        key_sel = prompt_norm[idx]                                  # [B, top_k, C]
        reduce_sim = torch.sum(key_sel * x_norm.unsqueeze(1)) / x_embed.shape[0]
        return {'prompt_idx': idx, 'prompt_norm': prompt_norm, 'x_embed_norm': x_norm,
                'similarity': similarity, 'selected_key': key_sel, 'reduce_sim': reduce_sim,
                'total_prompt_len': batched_prompt.shape[1],
                'prompted_embedding': torch.cat([batched_prompt, x_embed], dim=1)}
