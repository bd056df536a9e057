"""`LocPointTransformer` meta-architecture of the MQ task on the HIP path.

Reference: MQ/libs/modeling/meta_archs.py -- PtTransformerClsHead :183-275, PtTransformerRegHead
:278-349, PtTransformer :352-1736 (forward :753, preprocessing :1134, query_preprocessing :1184,
label_points_single_video :1253, losses :1374, inference_single_video :1594, postprocessing
:1695, Adapter :105-148, MemoryBank :38-60, BiasLayer :26-36).

Same constructor kwargs (`make_meta_arch('LocPointTransformer', **cfg['model'])`), same
`forward(video_list, ...)` contract (loss dict in training, list of per-video result dicts at
inference), same state_dict keys and the attributes / methods train_cl.py reads.  The dense work
(backbone, neck, heads) runs token-major on libvilco_hip.so; label assignment and the loss
reductions are [4536 x N] / [#valid x ncls] device tensor expressions under autograd.
"""
import math

import torch
from torch import nn
from torch.nn import functional as F

from .. import ops, switches
from ..cl_methods import CodaPrompt, Prompt
from ..utils.nms import batched_nms
from ..utils.model_ema import ModelEmaV2
from .blocks import LayerNorm, MaskedConv1D, Scale, from_tm, lens_to_mask, to_tm
from .losses import ctr_diou_loss_1d, sigmoid_focal_loss
from .models import make_backbone, make_generator, make_neck, register_meta_arch


def normal_distribution(x, mu=0, sigma=1):
    return (-(x - mu) ** 2 / (2 * sigma ** 2)).exp()


def _as_device(x, device):
    """cached distillation targets: device tensors as train_cl.cache_prev_logits keeps them here, or the reference's
    numpy arrays (train_cl.py:226-235)"""
    return x.to(device) if torch.is_tensor(x) else torch.from_numpy(x).to(device)


class BiasLayer(nn.Module):
    """BiC bias-correction layer (meta_archs.py:26-36)."""

    def __init__(self):
        super().__init__()
        self.alpha = nn.Parameter(torch.ones(1, requires_grad=True))
        self.beta = nn.Parameter(torch.zeros(1, requires_grad=True))

    def forward(self, x):
        return self.alpha * x + self.beta

    def printParam(self, i):
        print(i, self.alpha.item(), self.beta.item())


class MemoryBank:
    """ring buffer of narration embeddings for the SSL loss (meta_archs.py:38-60).  The write position lives on the device
    (`ring`, int32[1]): the fused SSL path advances it by a data-dependent count inside a launch, so a replayed step carries
    it; `ptr` reads it back (and waits for the device, like PtTransformer.loss_normalizer)."""

    def __init__(self, size, feature_dim, device=None):
        self.size, self.feature_dim = size, feature_dim
        self.memory = torch.randn(size, feature_dim, device=device if device is not None else "cuda")
        self.ring = torch.zeros(1, dtype=torch.int32, device=self.memory.device)

    @property
    def ptr(self):
        return int(self.ring.item())

    @ptr.setter
    def ptr(self, v):
        self.ring.fill_(int(v))

    @torch.no_grad()
    def update(self, features):
        n = features.size(0)
        assert n <= self.size, "Batch size must be less than or equal to memory bank size"
        ptr = self.ptr                       # one read of the device word per update
        end = ptr + n
        if end <= self.size:
            self.memory[ptr:end] = features
            self.ptr = end
        else:
            head = self.size - ptr
            self.memory[ptr:] = features[:head]
            self.memory[:end - self.size] = features[head:]
            self.ptr = end - self.size

    def get_all(self):
        return self.memory

    @torch.no_grad()
    def update_masked(self, features, mask):
        """rows of `features` [B, D] whose mask [B] is non-zero, in batch order, without a host read (ops.ssl_ring_update)"""
        ops.ssl_ring_update(features.detach(), mask.to(torch.float32), self.memory, self.ring)


class Adapter(nn.Module):
    """time-axis adapter of the ViLCo method (meta_archs.py:105-148): a Linear over the T axis,
    T -> 5T -> T/2, added in parallel to a stride-2 attention output."""

    def __init__(self, embed_dim, down_sample=5, mode="parallel", scale=None, act_layer=nn.GELU, stride=1):
        super().__init__()
        assert mode in ["before", "after", "parallel"], f"Unknown mode {mode}"
        hidden_dim = int(embed_dim * down_sample)
        self.layer = nn.Sequential(nn.Linear(embed_dim, hidden_dim), act_layer(),
                                   nn.Linear(hidden_dim, embed_dim // 2))
        self.mode = mode
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.layer[0].weight, a=math.sqrt(5))
        nn.init.zeros_(self.layer[0].bias)
        nn.init.zeros_(self.layer[2].weight)
        nn.init.zeros_(self.layer[2].bias)

    def forward_tm(self, x):
        """x [B,T,D] token-major -> [B,T/2,D]: the Linear acts on T, so run it channel-first."""
        if self.mode != "parallel":
            raise NotImplementedError("only the 'parallel' adapter mode is used (meta_archs.py:684)")
        xc = ops.transpose(x)                                           # [B,D,T]
        h = ops.linear(xc, self.layer[0].weight, self.layer[0].bias, ops.ACT_GELU)
        h = ops.linear(h, self.layer[2].weight, self.layer[2].bias)     # [B,D,T/2]
        return ops.transpose(h)


def freeze(module):
    for p in module.parameters():
        p.requires_grad_(False)
        p.grad = None


def unfreeze(module):
    for p in module.parameters():
        p.requires_grad_(True)


class _ConvHead(nn.Module):
    """[conv k3 -> LN -> ReLU] x (num_layers-1) shared across pyramid levels."""

    def _build(self, input_dim, feat_dim, num_layers, kernel_size, with_ln):
        self.head, self.norm = nn.ModuleList(), nn.ModuleList()
        for idx in range(num_layers - 1):
            self.head.append(MaskedConv1D(input_dim if idx == 0 else feat_dim, feat_dim, kernel_size,
                                          stride=1, padding=kernel_size // 2, bias=(not with_ln)))
            self.norm.append(LayerNorm(feat_dim) if with_ln else nn.Identity())

    def _trunk(self, x, lens):
        for conv, norm in zip(self.head, self.norm):
            x, _ = conv.forward_tm(x, lens)
            x = norm.forward_tm(x, relu=True) if isinstance(norm, LayerNorm) else torch.relu(x)
        return x

    # ---- all pyramid levels in one pass.  The head weights are shared across levels (meta_archs.py:216-235), so the
    # levels of each clip are laid end to end as ONE token sequence with a zero row between neighbours: a k=3 conv
    # over it equals the per-level convs (each level sees the zero padding it would get alone), the GEMMs get
    # M = B * sum(T_l) rows instead of six small problems, and every other kernel of the trunk runs once.
    # Rows beyond a level's valid length keep the reference's semantics (conv output * mask, then LN / ReLU of the
    # zero row); separator rows are forced back to zero after every layer.
    def _conv_cat(self, conv, x, cat):
        c = conv.conv
        assert c.kernel_size[0] == 3 and conv.stride == 1 and c.groups == 1
        if not _HEAD_ROWMASK:                        # (A/B: the mask as a separate multiply, as up to round 3)
            return ops.conv3(x, c.weight, c.bias, None) * cat.valid
        return ops.conv3(x, c.weight, c.bias, None, row_mask=cat.valid)          # output rows masked in the GEMM epilogue

    def _trunk_cat(self, x, cat):
        for conv, norm in zip(self.head, self.norm):
            x = self._conv_cat(conv, x, cat)
            if isinstance(norm, LayerNorm):
                # the separator rows are zeroed by the LayerNorm kernel itself, which also writes the next conv's operand image
                x = norm.forward_tm(x, relu=True, planes="seq", row_mask=cat.notgap)
            else:
                x = torch.relu(x)
        return x

    @staticmethod
    def can_cat(heads):
        return all(m.conv.kernel_size[0] == 3 and m.stride == 1 and m.conv.groups == 1 for m in heads)


_HEAD_ROWMASK = switches.on("VILCO_HEAD_ROWMASK")


class LevelCat:
    """Pyramid levels [B,T_l,C] of every clip concatenated along T with one zero row between levels."""

    _layout = {}     # (T_l ..., device) -> constant index tensors of the concatenated layout

    @classmethod
    def _get_layout(cls, Ts, dev):
        key = (tuple(Ts), str(dev))
        lay = cls._layout.get(key)
        if lay is None:
            off, lvl, pos, o = [], [], [], 0
            for i, T in enumerate(Ts):
                if i:
                    lvl.append(i); pos.append(1 << 30); o += 1          # separator row: never valid
                off.append(o)
                lvl.extend([i] * T); pos.extend(range(T)); o += T
            notgap = torch.tensor([0.0 if p_ == (1 << 30) else 1.0 for p_ in pos], dtype=torch.float32, device=dev)
            lay = (off, o, torch.tensor(lvl, dtype=torch.long, device=dev), torch.tensor(pos, dtype=torch.int32, device=dev),
                   notgap[None, :, None])
            cls._layout = {key: lay}
        return lay

    def __init__(self, feats, lens):
        B, dev = feats[0].shape[0], feats[0].device
        self.T = [f.shape[1] for f in feats]
        self.off, total, lvl, pos, self.notgap = self._get_layout(self.T, dev)
        zero = feats[0].new_zeros(B, 1, feats[0].shape[2])
        pieces = []
        for i, f in enumerate(feats):
            if i:
                pieces.append(zero)
            pieces.append(f)
        self.x = torch.cat(pieces, dim=1)
        lim = torch.stack([l.to(torch.int32) for l in lens], dim=1)[:, lvl]            # [B,Tc] valid length of the row's level
        self.valid = (pos[None, :] < lim).to(torch.float32)[:, :, None]                 # [B,Tc,1]

    def split(self, y):
        return [y[:, o:o + T] for o, T in zip(self.off, self.T)]


class PtTransformerClsHead(_ConvHead):
    def __init__(self, input_dim, feat_dim, num_classes, prior_prob=0.01, num_layers=3, kernel_size=3,
                 act_layer=nn.ReLU, with_ln=False, empty_cls=[], detach_feat=False):
        super().__init__()
        self.act = act_layer()
        self.detach_feat, self.num_classes = detach_feat, num_classes
        self._build(input_dim, feat_dim, num_layers, kernel_size, with_ln)
        self.cls_head = MaskedConv1D(feat_dim, num_classes, kernel_size, stride=1, padding=kernel_size // 2)
        torch.nn.init.constant_(self.cls_head.conv.bias, -(math.log((1 - prior_prob) / prior_prob)))
        if len(empty_cls) > 0:
            for idx in empty_cls:
                torch.nn.init.constant_(self.cls_head.conv.bias[idx], -(math.log((1 - 1e-6) / 1e-6)))
        self.reg_params = {}

    def augment_classification(self, num_new_classes, device):
        self.cls_head.augment_classification(num_new_classes, device)
        self.num_classes += num_new_classes

    def forward_tm(self, feats, lens, cat=None):
        """-> list of logits [B, T_l, ncls] (already the permuted layout of meta_archs.py:848)."""
        if cat is not None and self.can_cat(list(self.head) + [self.cls_head]):
            x = self._trunk_cat(cat.x.detach() if self.detach_feat else cat.x, cat)
            cat.cls_logits = self._conv_cat(self.cls_head, x, cat)       # [B, Tc, ncls]: the fused loss reads it whole
            return cat.split(cat.cls_logits)
        out = []
        for x, l in zip(feats, lens):
            x = self._trunk(x.detach() if self.detach_feat else x, l)
            out.append(self.cls_head.forward_tm(x, l)[0])
        return out

    def forward(self, fpn_feats, fpn_masks):
        lens = [m.reshape(m.shape[0], -1).sum(1).to(torch.int32) for m in fpn_masks]
        return tuple(from_tm(y) for y in self.forward_tm([to_tm(f) for f in fpn_feats], lens))


class PtTransformerRegHead(_ConvHead):
    def __init__(self, input_dim, feat_dim, fpn_levels, num_layers=3, kernel_size=3, act_layer=nn.ReLU,
                 with_ln=False, num_bins=16):
        super().__init__()
        self.fpn_levels = fpn_levels
        self.act = act_layer()
        self._build(input_dim, feat_dim, num_layers, kernel_size, with_ln)
        self.scale = nn.ModuleList([Scale() for _ in range(fpn_levels)])
        self.offset_head = MaskedConv1D(feat_dim, 2 * (num_bins + 1), kernel_size, stride=1,
                                        padding=kernel_size // 2)
        self.reg_params = {}

    def forward_tm(self, feats, lens, cat=None, raw=False):
        """raw=True (training with the fused loss kernel, which applies relu(Scale_l(x)) itself): only `cat.raw_offsets`
        [B, Tc, 2] is produced and None returned."""
        assert len(feats) == self.fpn_levels
        if cat is not None and self.can_cat(list(self.head) + [self.offset_head]):
            cat.raw_offsets = self._conv_cat(self.offset_head, self._trunk_cat(cat.x, cat), cat)
            if raw:
                return None
            off = cat.split(cat.raw_offsets)
            return [F.relu(self.scale[l](o)) for l, o in enumerate(off)]
        out = []
        for l, (x, ln) in enumerate(zip(feats, lens)):
            x = self._trunk(x, ln)
            off, _ = self.offset_head.forward_tm(x, ln)
            out.append(F.relu(self.scale[l](off)))       # [B, T_l, 2]: tiny, plain device ops
        return out

    def forward(self, fpn_feats, fpn_masks):
        lens = [m.reshape(m.shape[0], -1).sum(1).to(torch.int32) for m in fpn_masks]
        return tuple(from_tm(y) for y in self.forward_tm([to_tm(f) for f in fpn_feats], lens))


class StepInputs:
    """device-resident inputs of one step (PtTransformer.prepare): feats_cf [B,Cin,T], lens int32 [B], text_cf
    [B,Ctxt,L], text_lens int32 [B], gt float [B, 3*Nmax+1] (training); the narration inputs of the fused SSL path:
    narr_cf [B,Cn,n_pad] tokens, narr_lens int32 [B] token counts, narr_mask float [B] (the clip has a narration); narr =
    the unfused path's narration tuple or None; dist_tgt float [sum T_l, ldt] = the iCaRL / BiC distillation targets of the
    step (one cached clip's levels end to end, PtTransformer.distill_target) with dist_lens = (T_l, ...), or None; dist_kind =
    the method ('icarl' / 'bic') the caller that replays the step attached dist_tgt for (graph.GraphedStep._prepare), or None;
    der_tab int64 [B, 2] = (address of the row's DER record or 0, its class count) of a cl_name 'der' step
    (cl_methods.der.step_table), or None: the step then builds it from the clip list; pod_tab int64 [B] = the address of the
    row's POD record or 0 of a cl_name 'pod' step (cl_methods.pod.step_table), or None: likewise; erd_tab int64 [B, 5] = the
    addresses of the row's ERD maps and selected rows and its class count, or zeros, of a cl_name 'erd' step
    (cl_methods.erd.step_table), or None: likewise; ace_lo int32 [B] = the first class column the row's classification terms
    visit under cl_name 'er_ace' (cl_methods.ace.step_table), or None: likewise"""
    __slots__ = ("feats_cf", "lens", "T", "text_cf", "text_lens", "narr", "gt", "narr_cf", "narr_lens", "narr_mask",
                 "dist_tgt", "dist_lens", "dist_kind", "der_tab", "pod_tab", "erd_tab", "ace_lo")
    HOST = ("T", "narr", "dist_lens", "dist_kind")          # not device buffers: a captured step takes them over as they are

    def tensors(self):
        """(name, tensor) of every device buffer a replayed step reads"""
        return [(k, getattr(self, k)) for k in ("feats_cf", "lens", "text_cf", "text_lens", "gt", "narr_cf", "narr_lens",
                                                "narr_mask", "dist_tgt", "der_tab", "pod_tab", "erd_tab", "ace_lo")
                if getattr(self, k, None) is not None]

    def signature(self):
        return (tuple((k, tuple(t.shape)) for k, t in self.tensors()) + (("narr", self.narr is not None),) +
                (("dist_lens", getattr(self, "dist_lens", None)), ("dist_kind", getattr(self, "dist_kind", None))))


@register_meta_arch("LocPointTransformer")
class PtTransformer(nn.Module):
    def __init__(self, backbone_type, fpn_type, use_xl, backbone_arch, scale_factor, input_dim,
                 max_seq_len, max_buffer_len_factor, n_head, n_mha_win_size, embd_kernel_size, embd_dim,
                 embd_with_ln, fpn_dim, fpn_with_ln, fpn_start_level, head_dim, regression_range,
                 head_num_layers, head_kernel_size, head_with_ln, use_abs_pe, use_rel_pe, num_classes,
                 train_cfg, test_cfg, cl_cfg, use_cross_modal, n_txt_in, xlnet_config=None):
        super().__init__()
        self.fpn_strides = [scale_factor ** i for i in range(fpn_start_level, backbone_arch[-1] + 1)]
        self.reg_range = regression_range
        assert len(self.fpn_strides) == len(self.reg_range)
        self.scale_factor, self.num_classes, self.max_seq_len = scale_factor, num_classes, max_seq_len
        if isinstance(n_mha_win_size, int):
            self.mha_win_size = [n_mha_win_size] * (1 + backbone_arch[-1])
        else:
            assert len(n_mha_win_size) == (1 + backbone_arch[-1])
            self.mha_win_size = n_mha_win_size
        max_div_factor = 1
        for s, w in zip(self.fpn_strides, self.mha_win_size):
            stride = s * (w // 2) * 2 if w > 1 else s
            assert max_seq_len % stride == 0, "max_seq_len must be divisible by fpn stride and window size"
            max_div_factor = max(max_div_factor, stride)
        self.max_div_factor, self.use_xl = max_div_factor, use_xl

        t = train_cfg
        self.train_center_sample = t['center_sample']
        assert self.train_center_sample in ['radius', 'none']
        self.train_center_sample_radius = t['center_sample_radius']
        self.train_loss_weight, self.train_cls_prior_prob = t['loss_weight'], t['cls_prior_prob']
        self.train_dropout, self.train_droppath = t['dropout'], t['droppath']
        self.train_label_smoothing = t['label_smoothing']
        self.t_c_alpha, self.al_loss_weight = t['t_c_alpha'], t['al_loss_weight']
        self.cont_loss_weight, self.seg_loss_weight = t['cont_loss_weight'], t['seg_loss_weight']
        self.queue_size, self.temperature = t['queue_size'], t['temperature']
        self.use_dcn, self.dcn_start_layer, self.use_us_fpn = t['use_dcn'], t['dcn_start_layer'], t['use_us_fpn']
        self.length_theta, self.num_bins, self.iou_weight_power = t['length_theta'], t["num_bins"], t["iou_weight_power"]

        self.test_pre_nms_thresh, self.test_pre_nms_topk = test_cfg['pre_nms_thresh'], test_cfg['pre_nms_topk']
        self.test_iou_threshold, self.test_min_score = test_cfg['iou_threshold'], test_cfg['min_score']
        self.test_max_seg_num, self.test_nms_method = test_cfg['max_seg_num'], test_cfg['nms_method']
        assert self.test_nms_method in ['soft', 'hard', 'none']
        self.test_duration_thresh, self.test_multiclass_nms = test_cfg['duration_thresh'], test_cfg['multiclass_nms']
        self.test_nms_sigma, self.test_voting_thresh = test_cfg['nms_sigma'], test_cfg['voting_thresh']
        self.use_cross_modal, self.n_txt_in = use_cross_modal, n_txt_in

        assert backbone_type in ['convTransformer', 'conv']
        if backbone_type != 'convTransformer':
            raise NotImplementedError("backbone_type 'conv' is not used by any shipped MQ config")
        bb = {'n_in': input_dim, 'n_embd': embd_dim, 'n_head': n_head, 'n_embd_ks': embd_kernel_size,
              'max_len': max_seq_len, 'use_xl': use_xl, 'arch': backbone_arch, 't_c_alpha': self.t_c_alpha,
              'scale_factor': scale_factor, 'with_ln': embd_with_ln, 'attn_pdrop': 0.0,
              'proj_pdrop': self.train_dropout, 'path_pdrop': self.train_droppath, 'use_abs_pe': use_abs_pe,
              'use_rel_pe': use_rel_pe, 'use_dcn': self.use_dcn, 'dcn_start_layer': self.dcn_start_layer,
              'use_cross_modal': self.use_cross_modal, 'n_txt_in': self.n_txt_in}
        if xlnet_config is not None:
            bb['xlnet_config'] = xlnet_config
        self.backbone = make_backbone('convTransformer', **bb)
        if isinstance(embd_dim, (list, tuple)):
            embd_dim = sum(embd_dim)
        assert fpn_type in ['fpn', 'identity']
        self.neck = make_neck(fpn_type, **{'in_channels': [embd_dim] * (backbone_arch[-1] + 1),
                                           'out_channel': fpn_dim, 'scale_factor': scale_factor,
                                           'start_level': fpn_start_level, 'with_ln': fpn_with_ln,
                                           'use_us_fpn': self.use_us_fpn})
        self.point_generator = make_generator('point', **{'max_seq_len': max_seq_len * max_buffer_len_factor,
                                                           'fpn_strides': self.fpn_strides,
                                                           'regression_range': self.reg_range,
                                                           'use_us_fpn': self.use_us_fpn})
        self.cls_head = PtTransformerClsHead(fpn_dim, head_dim, self.num_classes, kernel_size=head_kernel_size,
                                             prior_prob=self.train_cls_prior_prob, with_ln=head_with_ln,
                                             num_layers=head_num_layers, empty_cls=t['head_empty_cls'])
        self.reg_head = PtTransformerRegHead(fpn_dim, head_dim, len(self.fpn_strides),
                                             kernel_size=head_kernel_size, num_layers=head_num_layers,
                                             with_ln=head_with_ln, num_bins=0)

        nc = self.num_classes
        self.mu = nn.Parameter(torch.zeros(nc, 1), requires_grad=True)
        self.sigma = nn.Parameter(torch.ones(nc, 1), requires_grad=True)
        self.mu_reg_left = nn.Parameter(-torch.ones(nc, 1) * 0.5, requires_grad=True)
        self.sigma_reg_left = nn.Parameter(torch.ones(nc, 1), requires_grad=True)
        self.mu_reg_right = nn.Parameter(torch.ones(nc, 1) * 0.5, requires_grad=True)
        self.sigma_reg_right = nn.Parameter(torch.ones(nc, 1), requires_grad=True)

        self.loss_normalizer = t['init_loss_norm']     # EMA, not checkpointed (:611); a device scalar in the sync-free path
        self._read_switches()
        self.loss_normalizer_momentum = 0.9
        self.reg_params = {}

        self.compute_means = cl_cfg['name'] == 'icarl'
        self.exemplar_means, self.memory = [], {}
        self.adv_lambda, self.type_sampling = cl_cfg['adv_lambda'], cl_cfg['type_sampling']
        self.n_known = 0
        self.dist_loss = nn.BCEWithLogitsLoss()
        self.list_bias_layers, self.list_splits = [], []
        self.bic_raw_logits = False          # True while cl_methods/bic.py caches the logits BEFORE the bias correction
        self.cl_name = cl_cfg['name']
        self.der_alpha = float(cl_cfg.get('der_alpha', 0.1))      # cl_name 'der' (cl_methods/der.py)
        self.der_bank = None                 # cl_methods.der.DERBank: the memory clips' insertion-time logits (train_cl.run_episodes)
        self.pod_lambda = float(cl_cfg.get('pod_lambda', 1.0))      # cl_name 'pod' (cl_methods/pod.py)
        self.pod_bank = None                 # cl_methods.pod.PODBank: the incoming model's pooled pyramid of the task's clips
        self._pod_step = None                # a get_emb pass of a 'pod' model leaves (pyramid, level lengths) here (pod.record_clips)
        from ..cl_methods import erd as _erd
        for k, v in _erd.OPTIONS.items():    # cl_name 'erd' (cl_methods/erd.py): erd_alpha_cls / _reg, erd_lambda_cls / _reg
            setattr(self, k, float(cl_cfg.get(k, v)))
        self.erd_bank = None                 # cl_methods.erd.ERDBank: the incoming model's confident responses on the task's clips

        self.prompt_pool = cl_cfg['prompt_pool']
        self.use_prompt_mask = True
        self.coda_ortho_mu = float(cl_cfg.get('coda_ortho_mu', 0.0))      # prompt_type 'coda' (cl_methods/coda.py)
        self._coda_ortho = None              # the step's penalty, from forward_prepared to _cl_terms
        prompt_type = cl_cfg.get('prompt_type', 'l2p')
        if prompt_type not in ('l2p', 'coda'):
            raise ValueError("cl_cfg.prompt_type must be 'l2p' or 'coda', got %r" % (prompt_type,))
        if cl_cfg['length'] is not None and cl_cfg['pool_size'] is not None and self.prompt_pool and prompt_type == 'coda':
            # ours: CODA-Prompt in the L2P pool's place.  Raises ValueError without coda_tasks or when it does not divide the pool
            self.prompt = CodaPrompt(cl_cfg['pool_size'], cl_cfg['length'], cl_cfg['embed_dim'], cl_cfg.get('coda_tasks'),
                                     ortho=self.coda_ortho_mu != 0.0, seed=cl_cfg.get('coda_seed', 0))
        elif cl_cfg['length'] is not None and cl_cfg['pool_size'] is not None and self.prompt_pool:
            self.prompt = Prompt(length=cl_cfg['length'], embed_dim=cl_cfg['embed_dim'], embedding_key='mean',
                                 prompt_init='uniform', prompt_pool=True, prompt_key=True,
                                 pool_size=cl_cfg['pool_size'], top_k=cl_cfg['topk'], batchwise_prompt=True,
                                 prompt_key_init='uniform')
        self.narration_ssl, self.narration_dim = cl_cfg["narration_ssl"], cl_cfg["narration_dim"]
        if self.narration_ssl:
            self.narration_encoder = nn.Linear(cl_cfg['narration_dim'], 1024)
            self._memory_bank_cfg = (cl_cfg['memory_size'], 1024)
            self.memory_bank = None        # created on first use, on the model's device
        self.ssl_factor = cl_cfg["ssl_factor"]

        self.num_emas, self.ema_decay = 1, 0.999
        self.use_adapt = cl_cfg['use_adapt']
        if self.use_adapt:
            self.adapt_blocks = cl_cfg['adapt_blocks']
            self.num_freeze_epochs = 10
            self.setup_adpat()

    def _read_switches(self):       # at construction: from __init__ and from the NLQ constructor, which does not run this class's
        self.level_cat = switches.on("VILCO_LEVEL_CAT")             # both heads over all pyramid levels at once (0: the per-level loop)
        self.sync_free_loss = switches.on("VILCO_SYNC_FREE_LOSS")
        self.fused_loss = switches.on("VILCO_FUSED_LOSS")           # ops.mq_loss (0: tensor expressions)
        self.fused_ssl = switches.on("VILCO_FUSED_SSL")             # ops.ssl_pool / ssl_nce (0: tensor expressions)

    # ------------------------------------------------------------------ adapters / EMA (ViLCo)
    def setup_adpat(self):
        if getattr(self, "pets_emas", None) is None:
            self.pets_emas = nn.ModuleList([])
            self.pets = self.create_pets()
        if len(self.pets_emas) < self.num_emas:
            self.pets_emas.append(ModelEmaV2(self.pets, decay=self.ema_decay))
        self.attach_pets(self.pets)

    def attach_pets(self, pets):
        for i, b in enumerate(self.adapt_blocks):
            self.backbone.branch[b].attach_adapter(attn=pets[i])

    def create_pets(self):
        pets, dim = nn.ModuleList([]), 1024          # hard-wired to T=1024 in the reference (:682)
        for _ in range(len(self.adapt_blocks)):
            pets.append(Adapter(embed_dim=dim, down_sample=5, mode='parallel', scale='null'))
            dim //= 2
        return pets

    def pre_train_epoch(self, task_id=0, current_epoch=0):
        unfreeze(self.pets)

    def post_train_step(self):
        for idx, ema in enumerate(reversed(self.pets_emas)):
            ema.update(self.pets if idx == 0 else self.pets_emas[idx - 1])

    @property
    def device(self):
        """the reference walks every parameter here (meta_archs.py:709-713; ~1 ms of host time per call at 465 tensors,
        several calls per step); all parameters live on one device, so the first one answers"""
        return self.mu.device

    def augment_classification(self, num_new_classes, device):
        device = self.mu.device
        self.cls_head.augment_classification(num_new_classes, device)
        old = self.num_classes
        self.num_classes += num_new_classes
        inits = {'mu': 0.0, 'sigma': 1.0, 'mu_reg_left': -0.5, 'sigma_reg_left': 1.0,
                 'mu_reg_right': 0.5, 'sigma_reg_right': 1.0}
        for name, val in inits.items():
            new = nn.Parameter(torch.full((self.num_classes, 1), val, device=device), requires_grad=True)
            new.data[:old] = getattr(self, name).data
            setattr(self, name, new)

    # ------------------------------------------------------------------ batching
    def _batch_cf(self, video_list, is_training=True, padding_val=0.0):
        """list of dicts -> (batched [B,C,T] channel-first on device, lens int32 [B], max_len)  (meta_archs.py:1134-1181)"""
        feats = [x['feats'] for x in video_list if len(x['labels']) > 0]
        feats_lens = [f.shape[-1] for f in feats]
        max_len = max(feats_lens)
        if is_training:
            assert max_len <= self.max_seq_len, "Input length must be smaller than max_seq_len during training"
            max_len = self.max_seq_len
        else:
            assert len(video_list) == 1, "Only support batch_size = 1 during inference"
            if max_len <= self.max_seq_len:
                max_len = self.max_seq_len
            else:
                stride = self.max_div_factor
                max_len = (max_len + (stride - 1)) // stride * stride
        dev = self.device
        batched = torch.full((len(feats), feats[0].shape[0], max_len), padding_val, dtype=torch.float32, device=dev)
        for f, dst in zip(feats, batched):
            dst[..., :f.shape[-1]].copy_(f, non_blocking=True)       # H2D (or D2D) of the raw [C, t_i]
        lens = self._h2d(torch.as_tensor(feats_lens, dtype=torch.int32))
        return batched, lens, max_len

    def preprocessing(self, video_list, is_training=True, padding_val=0.0):
        """list of dicts -> (x_tm [B,T,C] on device, lens int32 [B], max_len)  (meta_archs.py:1134-1181;
        the reference returns channel-first [B,C,T] + bool mask: see `preprocessing_cf`)."""
        batched, lens, max_len = self._batch_cf(video_list, is_training, padding_val)
        return ops.transpose(batched), lens, max_len

    def preprocessing_cf(self, video_list, is_training=True, padding_val=0.0):
        """reference-shaped return: (batched_inputs [B,C,T], batched_masks [B,1,T] bool, None)."""
        x_tm, lens, T = self.preprocessing(video_list, is_training, padding_val)
        return ops.transpose(x_tm), lens_to_mask(lens, T), None

    @torch.no_grad()
    def query_preprocessing(self, video_list, padding_val=0.0):
        """text tokens [768, L_i] -> token-major [B, Lmax, 768] + lens (meta_archs.py:1184-1221)."""
        batched, lens, narr = self._query_batch_cf(video_list, padding_val)
        return ops.transpose(batched), lens, narr

    def _ssl_fused(self, batch=1):
        """narration SSL through ops.ssl_pool / ops.ssl_nce: no host read, no boolean indexing, the ring pointer on the device.
        A batch outside the kernels' limits (include/vilco_hip.h: 1 <= B <= 64, B <= the bank's rows, D % 4 == 0, D <= 4096)
        takes the tensor-expression branch, as with VILCO_FUSED_SSL=0."""
        if not (self.narration_ssl and self.fused_ssl and self.sync_free_loss):
            return False
        M, D = self._memory_bank_cfg
        return 1 <= batch <= min(64, M) and D % 4 == 0 and D <= 4096

    @torch.no_grad()
    def _query_batch_cf(self, video_list, padding_val=0.0, narr_pad=8):
        """-> (batched [B,768,Lmax] channel-first on device, lens int32 [B], narration or None).  Narration: the tuple
        (tokens [B,Cn,n], m0 [B], m1 [B,1,n]) of the reference, or on the fused path the dict cf = tokens [B,Cn,n_pad]
        (zero-filled, n padded to a multiple of narr_pad so that the token count does not key a graph per batch), lens =
        int32 [B] token counts, mask = float [B]."""
        feats = [x['prompt_feature'] for x in video_list]
        lens_h = [f.shape[-1] for f in feats]
        dev = self.device
        batched = torch.full((len(feats), feats[0].shape[0], max(lens_h)), padding_val, dtype=torch.float32, device=dev)
        for f, dst in zip(feats, batched):
            dst[..., :f.shape[-1]].copy_(f, non_blocking=True)
        lens = self._h2d(torch.as_tensor(lens_h, dtype=torch.int32))
        narr = None
        if self.training and self._ssl_fused(len(video_list)):
            nf = [x['narration_feats'] for x in video_list]
            nl = [f.shape[-1] for f in nf]
            pad = max(int(narr_pad or 1), 1)
            nb = torch.zeros((len(nf), nf[0].shape[0], (max(nl) + pad - 1) // pad * pad), dtype=torch.float32, device=dev)
            for f, dst in zip(nf, nb):
                dst[..., :f.shape[-1]].copy_(f, non_blocking=True)
            narr = {'cf': nb, 'lens': self._h2d(torch.as_tensor(nl, dtype=torch.int32)),
                    'mask': self._h2d(torch.tensor([float(x['narration_mask']) for x in video_list], dtype=torch.float32))}
        elif self.training and self.narration_ssl:
            nf = [x['narration_feats'] for x in video_list]
            nl = [f.shape[-1] for f in nf]
            nb = torch.full((len(nf), nf[0].shape[0], max(nl)), padding_val, dtype=torch.float32, device=dev)
            for f, dst in zip(nf, nb):
                dst[..., :f.shape[-1]].copy_(f, non_blocking=True)
            m0 = torch.Tensor([x['narration_mask'] for x in video_list]).to(dev)
            m1 = (torch.arange(max(nl))[None, :] < torch.as_tensor(nl)[:, None]).unsqueeze(1).to(dev)
            narr = (nb, m0, m1)
        return batched, lens, narr

    def _gt_table(self, video_list, nmax=None):
        """ground truth of the labelled clips as ONE float table [B, 3*Nmax+1] for the fused label / loss kernels
        (include/vilco_hip.h: vilco_loss_desc.gt): 2*Nmax segment bounds, Nmax labels, the count.  Nmax may be padded
        (the kernels stop at the count), which keeps the table's shape stable from batch to batch."""
        vids = [x for x in video_list if len(x['labels']) > 0]
        n_real = max(int(x['labels'].shape[0]) for x in vids)
        nmax = n_real if nmax is None else max(int(nmax), n_real)
        gt = torch.zeros(len(vids), 3 * nmax + 1, dtype=torch.float32)
        for b, x in enumerate(vids):
            n = int(x['labels'].shape[0])
            gt[b, :2 * n] = x['segments'].reshape(-1).float().cpu()
            gt[b, 2 * nmax:2 * nmax + n] = x['labels'].float().cpu()
            gt[b, 3 * nmax] = n
        return self._h2d(gt)

    def _h2d(self, host):
        """small host table -> device without stalling the host: a copy from pageable memory waits for everything queued
        on the stream before it (one drained queue per step = the next step's ~1.6 ms of launches exposed, measured with
        tools/lab/replay_ab.py at config P); from a pinned staging block it is just another queued copy"""
        dev = self.device
        if dev.type == 'cuda':
            host = host.pin_memory()
        return host.to(dev, non_blocking=True)

    def prepare(self, video_list, is_training=True, gt_pad=None, narr_pad=8):
        """Everything `forward` takes from the clip dictionaries, as device tensors: the host half of the step (padding,
        H2D copies, the ground-truth table).  `forward_prepared` is the device half -- no host reads, no H2D copies, so a
        training step over a `StepInputs` can be captured as a hipGraph and replayed over refreshed buffers
        (vilco_amd/graph.py).  The channel-first -> token-major layout change is part of the device half."""
        inp = StepInputs()
        inp.feats_cf, inp.lens, inp.T = self._batch_cf(video_list, is_training)
        inp.text_cf = inp.text_lens = inp.narr = inp.narr_cf = inp.narr_lens = inp.narr_mask = None
        inp.dist_tgt = inp.dist_lens = inp.dist_kind = None        # filled by the caller that replays the step (graph.GraphedStep)
        inp.der_tab = inp.pod_tab = inp.erd_tab = inp.ace_lo = None
        if self.use_cross_modal:
            inp.text_cf, inp.text_lens, narr = self._query_batch_cf(video_list, narr_pad=narr_pad)
            if isinstance(narr, dict):
                inp.narr_cf, inp.narr_lens, inp.narr_mask = narr['cf'], narr['lens'], narr['mask']
                if self.memory_bank is None:       # before any capture: the bank is state, not a buffer of one step
                    self.memory_bank = MemoryBank(*self._memory_bank_cfg, device=self.device)
            else:
                inp.narr = narr
            assert inp.text_cf.shape[0] == inp.feats_cf.shape[0], \
                "every clip of the batch needs labels (the reference drops unlabelled clips from the video batch only)"
        inp.gt = None
        if is_training and video_list[0].get('segments') is not None and video_list[0].get('labels') is not None:
            inp.gt = self._gt_table(video_list, gt_pad)
        return inp

    # ------------------------------------------------------------------ forward
    def _run_network(self, x_tm, lens, text_tm, text_lens, raw_offsets=False):
        feats, all_lens = self.backbone.forward_tm(x_tm, lens, text_tm, text_lens)
        fpn_feats, fpn_lens = self.neck.forward_tm(feats, all_lens)
        cat = LevelCat(fpn_feats, fpn_lens) if (self.level_cat and len(fpn_feats) > 1) else None
        self._cat = cat
        if ops.fork_enabled("heads"):
            # the two heads share nothing but their input: the regression trunk runs on a side stream beside the
            # classification trunk (each of their k=3 convs is 1.5 rounds of tiles on 256 CUs: together 3 instead of 4)
            main, side = torch.cuda.current_stream(), ops.side_stream("heads", fpn_feats[0].device)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                out_offsets = self.reg_head.forward_tm(fpn_feats, fpn_lens, cat, raw=raw_offsets and cat is not None)
            out_cls_logits = self.cls_head.forward_tm(fpn_feats, fpn_lens, cat)
            main.wait_stream(side)
        else:
            out_offsets = self.reg_head.forward_tm(fpn_feats, fpn_lens, cat, raw=raw_offsets and cat is not None)
            out_cls_logits = self.cls_head.forward_tm(fpn_feats, fpn_lens, cat)
        return fpn_feats, fpn_lens, out_cls_logits, out_offsets

    def forward(self, video_list, task_id=-1, ensemble=False, hidden_state=False, is_training=True,
                prev_out_cls_logits=None, get_emb=False, val_qilDatasetList=None):
        inp = self.prepare(video_list, is_training)
        return self.forward_prepared(inp, video_list, task_id=task_id, ensemble=ensemble, is_training=is_training,
                                     prev_out_cls_logits=prev_out_cls_logits, get_emb=get_emb,
                                     val_qilDatasetList=val_qilDatasetList)

    def capturable(self, inp, task_id=-1, prev_out_cls_logits=None):
        """can forward_prepared(inp, None, task_id) + backward run without touching the host?  (the fused label / loss
        kernels, a prompt pool on ops.prompt_pool (or, with VILCO_FUSED_PROMPT=0, a fixed window), narration SSL only on its fused path -- the unfused one reads the mask sum and
        keeps the ring pointer on the host).  Distillation: an iCaRL step with n_known > 0 is capturable when its targets
        are resident on the device and travel in `inp.dist_tgt` (distill_target: the whole term is then ops.cl_distill
        over a buffer a replay refreshes); NumPy targets are uploaded per step and a batch without a cached clip has no
        target: those steps stay eager, and so does any other step that is handed targets.  A BiC step with n_known > 0
        needs the same of its targets -- attached FOR BiC (`inp.dist_kind`, set by GraphedStep._prepare) -- and a bias
        correction the device op takes (`_bic_op_ready`: one layer per split, the splits ending at the head's class count)
        with every layer on the model's device; its alpha / beta are read from memory by the replayed kernel."""
        if not (self.fused_loss and self.sync_free_loss and self.train_loss_weight > 0 and self.num_classes <= 128):
            return False
        if inp.gt is None:
            return False
        if self.training and self.narration_ssl and inp.narr_cf is None:
            return False
        if self.n_known > 0 and self.cl_name == 'icarl':
            if getattr(inp, "dist_tgt", None) is None:
                return False
        elif self.n_known > 0 and self.cl_name == 'bic':
            if getattr(inp, "dist_tgt", None) is None or getattr(inp, "dist_kind", None) != 'bic':
                return False
            if self.bic_raw_logits or not self._bic_op_ready():
                return False
            dev = self.device
            if any(p.device != dev for l in self.list_bias_layers for p in (l.alpha, l.beta)):
                return False
        elif self.n_known > 0 and self.cl_name == 'der':
            # the replayed term reads its records through the table in `inp.der_tab` (GraphedStep._prepare fills the slot)
            if getattr(inp, "der_tab", None) is None or prev_out_cls_logits:
                return False
        elif self.n_known > 0 and self.cl_name == 'pod':
            # likewise: the records are named by the table in `inp.pod_tab`
            if getattr(inp, "pod_tab", None) is None or prev_out_cls_logits:
                return False
        elif self.n_known > 0 and self.cl_name == 'erd':
            # likewise: the maps and the selected rows are named by the table in `inp.erd_tab`
            if getattr(inp, "erd_tab", None) is None or prev_out_cls_logits:
                return False
        elif self.n_known > 0 and self.cl_name == 'er_ace':
            # the replayed loss kernels read the clips' class windows from `inp.ace_lo` (GraphedStep._prepare fills the slot)
            if getattr(inp, "ace_lo", None) is None or prev_out_cls_logits:
                return False
        elif prev_out_cls_logits:
            return False
        if isinstance(getattr(self, 'prompt', None), CodaPrompt):
            # ops.coda_prompt reads nothing on the host; the tensor-op body slices by host integers only, but stays eager
            return bool(ops.fused_prompt and 0 <= task_id < self.prompt.n_tasks)
        if hasattr(self, 'prompt') and not (0 <= task_id and (task_id + 1) * self.prompt.top_k <= self.prompt.pool_size):
            # a task past the pool selects its prompts by similarity: only ops.prompt_pool does that without reading the host
            if not (ops.fused_prompt and task_id >= 0):
                return False
        return True

    def forward_prepared(self, inp, video_list=None, task_id=-1, ensemble=False, is_training=True,
                         prev_out_cls_logits=None, get_emb=False, val_qilDatasetList=None):
        """the device half of `forward` over a StepInputs; `video_list` is only needed by the paths that read the clip
        dictionaries (inference meta data, the unfused label path)."""
        x_tm, lens = ops.transpose(inp.feats_cf), inp.lens
        text_tm = text_lens = None
        narr = inp.narr
        # a step prepared for replay carries its distillation targets as one buffer; it wins over the lists it was made of
        self._dist_tgt = None if getattr(inp, "dist_tgt", None) is None else (inp.dist_tgt, inp.dist_lens)
        # a 'der' step: the table the caller attached, or the clips to build it from (_der_loss)
        self._der_step = (getattr(inp, "der_tab", None), video_list)
        self._pod_tab_step = (getattr(inp, "pod_tab", None), video_list)      # a 'pod' step: likewise (_pod_loss)
        self._erd_tab_step = (getattr(inp, "erd_tab", None), video_list)      # an 'erd' step: likewise (_erd_loss)
        self._ace_step = (getattr(inp, "ace_lo", None), video_list)      # an 'er_ace' step: likewise (_ace_window)
        if self.use_cross_modal:
            text_tm, text_lens = ops.transpose(inp.text_cf), inp.text_lens

        reduce_sim = None
        self._coda_ortho = None
        if isinstance(getattr(self, 'prompt', None), CodaPrompt):
            # CODA-Prompt: one weighted prompt of `length` tokens in front of the text; a task outside the pool's division
            # raises (ValueError) on the host while training, an eval forward uses every component up to the stored task's
            res = self.prompt(text_tm, task_id=task_id, train=is_training)
            self.total_prompt_len = res['total_prompt_len']
            text_tm = res['prompted_embedding']
            self._coda_ortho = res['ortho'] if is_training else None
        elif hasattr(self, 'prompt'):
            # L2P prompts are prepended to the text tokens (meta_archs.py:759-780).  The reference
            # rebuilds the mask over the first len(text) positions of the prompted sequence only.
            prompt_mask = None
            if is_training:
                start, end = task_id * self.prompt.top_k, (task_id + 1) * self.prompt.top_k
                if end <= self.prompt.pool_size:
                    # one device tensor per (window, B), kept: nothing is built per step and a captured step addresses it
                    prompt_mask = ops.prompt_window(start, self.prompt.top_k, text_tm.shape[0], text_tm.device)
            res = self.prompt(text_tm, prompt_mask=prompt_mask, cls_features=None)
            self.total_prompt_len = res['total_prompt_len']
            text_tm = res['prompted_embedding']                     # written contiguous by the op (and by torch.cat)
            reduce_sim = res['reduce_sim']

        # training with fixed loss weights: labels + losses are ONE fused kernel pair (ops.mq_loss) that also applies the
        # regression head's relu(Scale_l(x)); everything else (dynamic loss weight, get_emb, eval, a BiC correction the device
        # op does not take: a CPU model, a split table that does not end at the class count) keeps the lists
        bic_loop = (self.n_known > 0 and self.cl_name == 'bic' and not self.bic_raw_logits
                    and not (x_tm.is_cuda and self._bic_op_ready()))
        fused = (is_training and not get_emb and self.fused_loss and self.sync_free_loss and self.train_loss_weight > 0
                 and not bic_loop and self.num_classes <= 128)
        fpn_feats, fpn_lens, out_cls_logits, out_offsets = self._run_network(x_tm, lens, text_tm, text_lens,
                                                                            raw_offsets=fused)

        # the fused loss writes the memory bank and advances its ring word: only where the loss is consumed (the reference
        # touches the bank inside the training-loss branch, :939-945 -- not in a get_emb pass such as cache_prev_logits')
        ssl_fused = bool(self.training and inp.narr_cf is not None and is_training and not get_emb)
        if ssl_fused:
            ssl_loss = self._fused_ssl_loss(fpn_feats, fpn_lens, inp)
        elif self.training and self.narration_ssl and inp.narr_cf is None:
            narration_feats, video_feats = self._ssl_embeddings(fpn_feats, fpn_lens, narr)

        level_T = [f.shape[1] for f in fpn_feats]
        points = self.point_generator(fpn_feats, lengths=level_T)

        if self.n_known > 0 and self.cl_name == 'bic' and not self.bic_raw_logits:
            out_cls_logits = self._bic_correct_levels(out_cls_logits)

        # [B, T_l] bool per level -- not needed by the fused training losses (they read the prefix lengths): 12 launches less on the
        # chain of a captured step (round 6)
        fpn_masks = (None if (is_training and fused and not get_emb)
                     else [lens_to_mask(l, T).squeeze(1) for l, T in zip(fpn_lens, level_T)])

        if not is_training and self.use_adapt:
            # average with the prediction of every adapter EMA (meta_archs.py:854-881)
            for ema in self.pets_emas:
                self.attach_pets(ema.module)
                _, _, e_cls, e_off = self._run_network(x_tm, lens, text_tm, text_lens)
                out_cls_logits = [(a + b) / 2 for a, b in zip(out_cls_logits, e_cls)]
                out_offsets = [(a + b) / 2 for a, b in zip(out_offsets, e_off)]
            self.attach_pets(self.pets)

        if get_emb:
            if self.cl_name == 'pod':      # the pyramid of this pass, for cl_methods.pod.record_clips
                self._pod_step = (list(fpn_feats), torch.stack([l.to(torch.int32) for l in fpn_lens], dim=1).contiguous())
            return out_cls_logits, out_offsets, fpn_masks

        if is_training:
            assert inp.gt is not None, "GT action labels does not exist"
            dev = self.device
            if fused:
                losses = self._fused_losses(inp.gt, points, fpn_lens, out_cls_logits, out_offsets,
                                            prev_out_cls_logits, reduce_sim, fpn_feats=fpn_feats)
            else:
                gt_segments = [x['segments'].to(dev) for x in video_list if len(x['labels']) > 0]
                gt_labels = [x['labels'].to(dev) for x in video_list if len(x['labels']) > 0]
                gt_cls, gt_off, np_cls, np_reg = self.label_points(points, gt_segments, gt_labels)
                losses = self.losses(fpn_masks, out_cls_logits, out_offsets, gt_cls, gt_off, label_list=gt_labels,
                                     normal_probs_cls=np_cls, normal_probs_reg=np_reg,
                                     prev_out_cls_logits=prev_out_cls_logits, reduce_sim=reduce_sim, fpn_feats=fpn_feats)
            if ssl_fused:
                # always present on this path, an exact 0 when no clip of the batch has a narration (the reference leaves
                # the key out there: the sum is the same)
                losses["final_loss"] = losses["final_loss"] + self.ssl_factor * ssl_loss
                losses["ssl_loss"] = self.ssl_factor * ssl_loss
            elif self.narration_ssl and narr is not None and narr[1].sum() > 0:
                m0 = narr[1].to(torch.bool)
                self.memory_bank.update(narration_feats[m0])
                ssl_loss = self.masked_contrastive_loss(narration_feats, video_feats, m0)
                # (not in place: with the fused loss kernel final_loss is one of several views of its output, which autograd
                # refuses to modify -- the reference's `+=` raised on this path)
                losses["final_loss"] = losses["final_loss"] + self.ssl_factor * ssl_loss
                losses["ssl_loss"] = self.ssl_factor * ssl_loss
            return losses

        results = self.inference(video_list, points, fpn_masks, out_cls_logits, out_offsets, None, None,
                                 val_qilDatasetList)
        if ensemble:
            return video_list, points, fpn_masks, out_cls_logits, out_offsets
        return results

    def _bic_op_ready(self):
        """the bias layers are something ops.bic_correct takes: one layer per split and the splits ending at the head's class
        count (<= 128).  Anything else is the reference's slice-and-concatenate loop, whatever it makes of such a table."""
        n, n_classes = len(self.list_splits), self.cls_head.cls_head.conv.out_channels
        return 0 < n == len(self.list_bias_layers) and int(self.list_splits[-1]) == n_classes <= 128

    def _bic_correct_levels(self, levels):
        """the per-level list of head outputs, corrected (meta_archs.py:821-836).  On the device with the heads run over the
        LevelCat layout this is ONE ops.bic_correct launch over the concatenated logits, which the fused loss and the
        distillation term then read (`cat.cls_logits`); the levels are views of its result.  Out of place: the raw buffer is
        left as the head wrote it."""
        cat = self._cat
        if (levels[0].is_cuda and self._bic_op_ready() and cat is not None
                and getattr(cat, "cls_logits", None) is not None):
            cat.cls_logits = ops.bic_correct(cat.cls_logits, self.list_splits, self.list_bias_layers)
            return cat.split(cat.cls_logits)
        return [self._bic_correct(x) for x in levels]

    def _bic_correct(self, logits):
        """one tensor [..., ncls]: the device op where it applies, the reference's Python loop on a CPU model"""
        if logits.is_cuda and self._bic_op_ready():
            return ops.bic_correct(logits, self.list_splits, self.list_bias_layers)
        parts, lo = [], 0
        for i, hi in enumerate(self.list_splits):
            parts.append(self.list_bias_layers[i](logits[..., lo:hi]))
            lo = hi
        return torch.cat(parts, dim=-1)

    def _fused_ssl_loss(self, fpn_feats, fpn_lens, inp):
        """meta_archs.py:794-811 + 939-945 + 1351-1372 on the device: the narration encoder over the token-major tokens,
        both masked mean poolings (ops.ssl_pool), then normalisation, the bank's ring update and InfoNCE (ops.ssl_nce)"""
        if self.memory_bank is None:
            self.memory_bank = MemoryBank(*self._memory_bank_cfg, device=self.device)
        enc = self.narration_encoder
        tokens = ops.linear(ops.transpose(inp.narr_cf), enc.weight, enc.bias)                  # [B, n_pad, D]
        text = ops.ssl_pool([tokens], inp.narr_lens.reshape(-1, 1))
        level_len = torch.stack([l.to(torch.int32) for l in fpn_lens], dim=1).contiguous()     # as _fused_losses' table
        video = ops.ssl_pool(list(fpn_feats), level_len)
        bank = self.memory_bank
        return ops.ssl_nce(text, video, inp.narr_mask, bank.memory, bank.ring)[0]

    def _ssl_embeddings(self, fpn_feats, fpn_lens, narr):
        """masked mean pooling of narration / pyramid features (meta_archs.py:794-811)."""
        nb, m0, m1 = narr
        if self.memory_bank is None:
            self.memory_bank = MemoryBank(*self._memory_bank_cfg, device=self.device)
        nf = self.narration_encoder(nb.permute(0, 2, 1)).permute(0, 2, 1) * m1
        denom = torch.sum(m1, dim=2, dtype=torch.float)
        denom[denom == 0.] = 1.
        narration_feats = F.normalize(torch.sum(nf, dim=2) / denom, dim=1)
        pooled = []
        for f, l in zip(fpn_feats, fpn_lens):
            m = lens_to_mask(l, f.shape[1]).squeeze(1).to(f.dtype)             # [B,T]
            d = m.sum(1, keepdim=True)
            d[d == 0.] = 1.
            pooled.append((f * m.unsqueeze(-1)).sum(1) / d)
        video_feats = F.normalize(torch.stack(pooled).mean(0), dim=1)
        return narration_feats, video_feats

    def masked_contrastive_loss(self, text_embeddings, video_embeddings, mask, temperature=0.07):
        t, v = text_embeddings[mask], video_embeddings[mask]
        pos = torch.einsum('nc,nc->n', [t, v]).unsqueeze(-1)
        mem = self.memory_bank.get_all()
        lt = torch.cat([pos, t @ mem.T], dim=1) / temperature
        lv = torch.cat([pos, v @ mem.T], dim=1) / temperature
        labels = torch.zeros(t.size(0), dtype=torch.long, device=t.device)
        return (F.cross_entropy(lt, labels) + F.cross_entropy(lv, labels)) / 2

    # ------------------------------------------------------------------ labels
    def label_points(self, points, gt_segments, gt_labels, for_seg=False):
        concat_points = torch.cat(points, dim=0)
        gt_cls, gt_offset, np_cls, np_reg = [], [], [], []
        for seg, lab in zip(gt_segments, gt_labels):
            cls_t, reg_t, (p_cls, p_l, p_r) = self.label_points_single_video(concat_points, seg, lab)
            gt_cls.append(cls_t.detach())
            gt_offset.append(reg_t.detach())
            np_cls.append(p_cls)
            np_reg.append([p_l, p_r])
        return gt_cls, gt_offset, np_cls, np_reg

    def label_points_single_video(self, concat_points, gt_segment, gt_label):
        """all-pairs point/GT assignment with gaussian weights from the learnable mu/sigma
        (meta_archs.py:1253-1344)."""
        num_pts, num_gts = concat_points.shape[0], gt_segment.shape[0]
        if num_gts == 0:
            return gt_segment.new_full((num_pts, self.num_classes), 0), gt_segment.new_zeros((num_pts, 2))
        t = concat_points[:, 0, None]
        stride = concat_points[:, 3, None]
        lens = (gt_segment[:, 1] - gt_segment[:, 0])[None, :].repeat(num_pts, 1)
        left = t - gt_segment[None, :, 0]
        right = gt_segment[None, :, 1] - t
        rel = ((right - left) / 2.0) / (stride * lens)

        def gauss(mu, sigma):
            return normal_distribution(rel, mu[gt_label].permute(1, 0), sigma[gt_label].permute(1, 0))
        p_cls = gauss(self.mu, self.sigma)
        p_left = gauss(self.mu_reg_left, self.sigma_reg_left)
        p_right = gauss(self.mu_reg_right, self.sigma_reg_right)
        reg_targets = torch.stack((left, right), dim=-1)

        if self.train_center_sample == 'radius':
            center = 0.5 * (gt_segment[None, :, 0] + gt_segment[None, :, 1])
            t_mins = center - stride * self.train_center_sample_radius
            t_maxs = center + stride * self.train_center_sample_radius
            cb_left = t - torch.maximum(t_mins, gt_segment[None, :, 0])
            cb_right = torch.minimum(t_maxs, gt_segment[None, :, 1]) - t
            inside = torch.minimum(cb_left, cb_right) > 0
        else:
            inside = reg_targets.min(-1)[0] > 0
        max_dist = reg_targets.max(-1)[0]
        in_range = torch.logical_and(max_dist >= concat_points[:, 1, None], max_dist <= concat_points[:, 2, None])
        lens = lens.masked_fill(inside == 0, float('inf')).masked_fill(in_range == 0, float('inf'))
        min_len, min_len_inds = lens.min(dim=1)
        min_len_mask = torch.logical_and(lens <= (min_len[:, None] + 1e-3), lens < float('inf')).to(reg_targets.dtype)
        one_hot = F.one_hot(gt_label, self.num_classes).to(reg_targets.dtype)
        cls_targets = (min_len_mask @ one_hot).clamp_(min=0.0, max=1.0)
        rows = torch.arange(num_pts, device=concat_points.device)
        reg_targets = reg_targets[rows, min_len_inds] / stride
        return cls_targets, reg_targets, (p_cls[rows, min_len_inds], p_left[rows, min_len_inds],
                                          p_right[rows, min_len_inds])

    # ------------------------------------------------------------------ fused labels + losses
    def _loss_tables(self, points, cat, dev):
        """(points [R,4], row_level [R], row_pos [R]) of the row layout the loss kernel walks: the LevelCat layout with
        separator rows (stride 0) or the plain concatenation of the levels.  Cached per layout."""
        key = (tuple(p.shape[0] for p in points), cat is not None, str(dev))
        tab = getattr(self, "_loss_tab", None)
        if tab is None or tab[0] != key:
            rows, lvl, pos = [], [], []
            for i, p in enumerate(points):
                if i and cat is not None:
                    rows.append(p.new_zeros(1, 4))
                    lvl.append(i)
                    pos.append(1 << 30)
                rows.append(p)
                lvl.extend([i] * p.shape[0])
                pos.extend(range(p.shape[0]))
            tab = (key, (torch.cat(rows).contiguous().to(dev), torch.tensor(lvl, dtype=torch.int32, device=dev),
                         torch.tensor(pos, dtype=torch.int32, device=dev)))
            self._loss_tab = tab
        return tab[1]

    def _fused_losses(self, gt, points, fpn_lens, out_cls_logits, out_offsets, prev_out_cls_logits, reduce_sim, fpn_feats=None):
        """meta_archs.py:1253-1344 + 1374-1447 through ops.mq_loss; the CL terms (:1478-1519) are added on top.
        gt: the table of `_gt_table` -- one row per clip of the batch, in batch order."""
        cat, self._cat = self._cat, None       # not kept: it holds this step's head tensors and their autograd graph
        dev = self.device
        if cat is not None and getattr(cat, "raw_offsets", None) is not None and out_offsets is None:
            logits, offsets = cat.cls_logits, cat.raw_offsets
            scale = torch.stack([s.scale for s in self.reg_head.scale])
        else:
            logits, offsets, scale, cat = torch.cat(out_cls_logits, dim=1), torch.cat(out_offsets, dim=1), None, None
        assert gt.shape[0] == logits.shape[0], "ground-truth rows (%d) != clips in the batch (%d)" % (gt.shape[0], logits.shape[0])
        tables = self._loss_tables(points, cat, dev)
        level_len = torch.stack([l.to(torch.int32) for l in fpn_lens], dim=1).contiguous()
        gauss = torch.cat([self.mu, self.sigma, self.mu_reg_left, self.sigma_reg_left, self.mu_reg_right,
                           self.sigma_reg_right], dim=1).t().contiguous()                         # [6, ncls]
        norm = self._loss_norm
        if not (torch.is_tensor(norm) and norm.dim() == 1):
            norm = torch.full((1,), float(norm), dtype=torch.float32, device=dev)
            self._loss_norm = norm
        radius = self.train_center_sample_radius if self.train_center_sample == 'radius' else 0.0
        ace_lo = self._ace_window()
        if ace_lo is not None:       # cl_name 'er_ace' with known classes: the same kernels over the clips' class windows
            cls_loss, reg_loss, al_loss, final_loss = ops.mq_loss_ace(
                logits, offsets, scale, gauss, tables, level_len, gt, norm, radius, self.train_label_smoothing,
                self.loss_normalizer_momentum, self.train_loss_weight, self.al_loss_weight, logits.shape[-1] != 1, ace_lo)
        else:
            cls_loss, reg_loss, al_loss, final_loss = ops.mq_loss(
                logits, offsets, scale, gauss, tables, level_len, gt, norm, radius, self.train_label_smoothing,
                self.loss_normalizer_momentum, self.train_loss_weight, self.al_loss_weight, logits.shape[-1] != 1)
        level_T = [int(p.shape[0]) for p in points]
        level_row = cat.off if cat is not None else [sum(level_T[:i]) for i in range(len(level_T))]
        return self._cl_terms({'cls_loss': cls_loss, 'reg_loss': reg_loss, 'al_loss': al_loss}, final_loss,
                              out_cls_logits, prev_out_cls_logits, reduce_sim, cat_logits=(logits, level_row),
                              level_len=level_len, fpn_feats=fpn_feats, cat_offsets=(offsets, scale))

    def _ace_window(self):
        """cl_name 'er_ace' (ours; cl_methods/ace.py) with known classes: int32 [B], the first class column each clip's
        classification terms visit -- the table the caller attached (StepInputs.ace_lo) or one built from the step's clips;
        None for every other step, which takes the plain loss."""
        (tab, video_list), self._ace_step = getattr(self, "_ace_step", None) or (None, None), None
        if not (self.n_known > 0 and self.cl_name == 'er_ace'):
            return None
        if tab is None:
            if video_list is None:
                raise ValueError("a cl_name 'er_ace' step needs StepInputs.ace_lo or the list of its clips")
            from ..cl_methods import ace
            tab = ace.step_table(self, video_list)
        return tab

    # ------------------------------------------------------------------ losses
    @property
    def loss_normalizer(self):
        """python float like the reference's attribute; reading it after a sync-free step waits for the device."""
        v = self._loss_norm
        return float(v) if torch.is_tensor(v) else v

    @loss_normalizer.setter
    def loss_normalizer(self, v):
        self._loss_norm = float(v)

    def _loss_norm_tensor(self, device):
        v = self._loss_norm
        return v.reshape(()) if torch.is_tensor(v) else torch.tensor(float(v), dtype=torch.float32, device=device)

    def losses(self, fpn_masks, out_cls_logits, out_offsets, gt_cls_labels, gt_offsets, label_list=None,
               normal_probs_cls=None, normal_probs_reg=None, out_importances=None, out_start=None,
               out_end=None, prev_out_cls_logits=None, stage_id=0, reduce_sim=None, fpn_feats=None):
        """focal + DIoU with gaussian point weights, 'al' loss, CL distillation terms
        (meta_archs.py:1374-1524).  One host sync: num_pos (as in the reference, :1407)."""
        valid_mask = torch.cat(fpn_masks, dim=1)
        gt_cls = torch.stack(gt_cls_labels)
        w_cls = torch.stack(normal_probs_cls)
        w_left = torch.stack([x[0] for x in normal_probs_reg])
        w_right = torch.stack([x[1] for x in normal_probs_reg])
        pos_mask = torch.logical_and((gt_cls.sum(-1) > 0), valid_mask)
        logits_all = torch.cat(out_cls_logits, dim=1)
        offsets_all = torch.cat(out_offsets, dim=1)
        gt_off_all = torch.stack(gt_offsets)
        gt_target = gt_cls * (1 - self.train_label_smoothing) + self.train_label_smoothing / (self.num_classes + 1)
        w_cls = torch.where(pos_mask, w_cls, torch.ones_like(w_cls))           # negatives weigh 1
        # cl_name 'er_ace' with known classes (ours; cl_methods/ace.py): bool [B, 1, C], the class columns each clip's
        # classification terms visit -- what ops.mq_loss_ace does in the kernels, in tensor ops
        ace_lo, ace_cols = self._ace_window(), None
        if ace_lo is not None:
            from ..cl_methods import ace
            ace_cols = ace.column_mask(ace_lo.to(logits_all.device), logits_all.shape[-1]).unsqueeze(1)

        if self.sync_free_loss:
            # Same sums as the reference, evaluated densely over all points with 0/1 weights instead of boolean
            # gathers: no host round trip anywhere in the step (the reference syncs on num_pos, on every boolean
            # index and in the DIoU asserts), so the GPU never waits for the host between forward and backward.
            num_pos = pos_mask.sum()
            norm = self._loss_norm_tensor(logits_all.device)
            norm = self.loss_normalizer_momentum * norm + (1 - self.loss_normalizer_momentum) * num_pos.clamp(min=1).to(norm.dtype)
            self._loss_norm = norm.detach()
            vf, pf = valid_mask.to(logits_all.dtype), pos_mask.to(logits_all.dtype)
            cls_loss = sigmoid_focal_loss(logits_all, gt_target, reduction='None')
            if ace_cols is not None:
                cls_loss = cls_loss * ace_cols.to(cls_loss.dtype)
            cls_loss = (cls_loss.sum(-1) * w_cls * vf).sum() / norm
            one = torch.ones_like(gt_off_all)
            reg = ctr_diou_loss_1d(torch.where(pos_mask[..., None], offsets_all, one).reshape(-1, 2),
                                   torch.where(pos_mask[..., None], gt_off_all, one).reshape(-1, 2),
                                   reduction='None', check=False).reshape(pos_mask.shape)
            reg_loss = (reg * ((w_left + w_right) / 2.0) * w_cls * pf).sum() / norm
        else:
            pred_offsets = offsets_all[pos_mask]
            gt_off = gt_off_all[pos_mask]
            num_pos = pos_mask.sum().item()
            self.loss_normalizer = self.loss_normalizer_momentum * self.loss_normalizer + (
                1 - self.loss_normalizer_momentum) * max(num_pos, 1)
            norm = self.loss_normalizer
            cls_loss = sigmoid_focal_loss(logits_all[valid_mask], gt_target[valid_mask], reduction='None')
            if ace_cols is not None:
                cls_loss = cls_loss * ace_cols.expand_as(logits_all)[valid_mask].to(cls_loss.dtype)
            cls_loss = (cls_loss.sum(-1) * w_cls[valid_mask]).sum() / norm
            if num_pos == 0:
                reg_loss = 0 * pred_offsets.sum()
            else:
                reg_loss = ctr_diou_loss_1d(pred_offsets, gt_off, reduction='None')
                reg_loss = reg_loss * ((w_left[pos_mask] + w_right[pos_mask]) / 2.0) * w_cls[pos_mask]
                reg_loss = reg_loss.sum() / norm

        if label_list is not None and (out_cls_logits[0].shape[-1] != 1):
            score = logits_all.masked_fill(valid_mask.unsqueeze(-1) == False, -1e7)   # noqa: E712
            if ace_cols is not None:       # the softmax of a clip's rows is over its window: a masked row scores 1 / (C - lo)
                score = score.masked_fill(~ace_cols, float('-inf'))
            score = torch.max(score.softmax(-1), dim=1)[0]
            involved = torch.zeros_like(score)
            for i in range(involved.shape[0]):
                involved[i, label_list[i]] = 1
            if ace_cols is not None:
                # the masked sum, one logarithm per (clip, class) as in the kernels: of the score for an involved class, of its
                # complement otherwise (a window of one class scores exactly 1: 0 * log(0) must not enter); the columns below
                # the window (score 0) take 1 and add -log(1) = 0
                q = torch.where(involved > 0, score, 1 - score)
                al_loss = -torch.where(ace_cols.squeeze(1), q, torch.ones_like(q)).log().sum() / norm
            else:
                al_loss = (-involved * score.log() - (1 - involved) * (1 - score).log()).sum() / norm
        else:
            al_loss = torch.zeros((1,), device=cls_loss.device)

        if self.train_loss_weight > 0:
            loss_weight = self.train_loss_weight
        else:
            loss_weight = cls_loss.detach() / max(reg_loss.item(), 0.01)
        final_loss = cls_loss + reg_loss * loss_weight + al_loss * self.al_loss_weight

        level_T = [int(x.shape[1]) for x in out_cls_logits]
        return self._cl_terms({'cls_loss': cls_loss, 'reg_loss': reg_loss, 'al_loss': al_loss}, final_loss, out_cls_logits,
                              prev_out_cls_logits, reduce_sim,
                              cat_logits=(logits_all, [sum(level_T[:i]) for i in range(len(level_T))]),
                              level_len=torch.stack([m.sum(1) for m in fpn_masks], dim=1).to(torch.int32).contiguous()
                              if self.cl_name in ('der', 'pod', 'erd') else None, fpn_feats=fpn_feats,
                              cat_offsets=(offsets_all, None))

    @staticmethod
    def _icarl_levels(prev_out_cls_logits, len_f):
        """the reference's choice of iCaRL targets (meta_archs.py:1505-1506): handed a list over the batch's cached clips, the
        first clip's per-level list"""
        if len(prev_out_cls_logits) != len_f or len(prev_out_cls_logits) == 1:
            return prev_out_cls_logits[0]
        return prev_out_cls_logits

    def distill_target(self, prev_out_cls_logits):
        """-> (buffer [sum T_l, ldt], (T_l, ...)): the iCaRL / BiC targets a step with these cached outputs distils against,
        as the one contiguous device buffer ops.cl_distill reads (train_cl.cache_prev_logits stores a clip's levels as views
        of such a buffer: nothing is copied then).  iCaRL is handed the list over the batch's cached clips and takes the
        first; BiC is handed ONE clip's per-level list (train_one_epoch: the last cached clip's).  None when there is
        nothing a replayed step could carry: not an iCaRL / BiC step with known classes, no cached clip in the batch, or
        host-side (NumPy) targets."""
        if not (self.n_known > 0 and self.cl_name in ('icarl', 'bic') and prev_out_cls_logits):
            return None
        if self.cl_name == 'bic':
            levels = prev_out_cls_logits
            if len(levels) != len(self.fpn_strides):
                return None
        else:
            levels = self._icarl_levels(prev_out_cls_logits, len(self.fpn_strides))
        if not all(torch.is_tensor(t) and t.is_cuda for t in levels):
            return None
        return ops.distill_targets(levels, self.device)

    def _device_distill(self, out_cls_logits, prev_out_cls_logits, cat_logits):
        """both distillation terms as ONE ops.cl_distill call (csrc/distill.hip) over the concatenated head output"""
        bic = self.cl_name == 'bic'
        level_T = tuple(int(x.shape[1]) for x in out_cls_logits)
        tgt, self._dist_tgt = getattr(self, "_dist_tgt", None), None
        if tgt is None:
            levels = prev_out_cls_logits if bic else self._icarl_levels(prev_out_cls_logits, len(level_T))
            if len(levels) != len(level_T):
                raise ValueError("distillation targets of %d levels for a pyramid of %d" % (len(levels), len(level_T)))
            tgt = ops.distill_targets(levels, out_cls_logits[0].device)
        targets, lens = tgt
        if tuple(lens) != level_T:
            raise ValueError("the distillation targets' level lengths %s differ from the logits' %s (cached with another "
                             "max_seq_len?)" % (tuple(lens), level_T))
        if targets.shape[1] < self.n_known:
            raise ValueError("the distillation targets hold %d classes, n_known is %d" % (targets.shape[1], self.n_known))
        logits, level_row = cat_logits if cat_logits is not None else (list(out_cls_logits), None)
        n_classes = self.cls_head.cls_head.conv.out_channels
        return ops.cl_distill(logits, level_row, level_T, targets, self.n_known,
                              ops.DISTILL_BIC if bic else ops.DISTILL_ICARL, 0.01 * self.n_known / n_classes)

    def _der_levels(self):
        """the level lengths of a training step (every batch is padded to max_seq_len): what a usable DER record was made with"""
        return tuple(self.max_seq_len // s for s in self.fpn_strides)

    def _der_loss(self, out_cls_logits, cat_logits, level_len):
        """cl_name 'der' (ours; cl_methods/der.py): der_alpha * mean (x - z)^2 over the memory clips of the batch against their
        insertion-time logits.  On the device ONE ops.der_replay call (csrc/der.hip) over the concatenated head output, the
        records named by a device table; a CPU model evaluates the same term in tensor ops."""
        from ..cl_methods import der
        (tab, video_list), self._der_step = getattr(self, "_der_step", None) or (None, None), None
        logits, level_row = cat_logits
        level_T = tuple(int(x.shape[1]) for x in out_cls_logits)
        if logits.is_cuda:
            if tab is None:
                if video_list is None:
                    raise ValueError("a cl_name 'der' step needs StepInputs.der_tab or the list of its clips")
                tab = der.step_table(self, video_list, level_T)
            return ops.der_replay(logits, level_row, level_T, level_len, tab, self.der_alpha)
        if video_list is None:
            raise ValueError("a cl_name 'der' step on a CPU model needs the list of its clips")
        vids, bank = der.labelled(video_list), self.der_bank
        rows = bank.rows_for(vids, [der.clip_len(v) for v in vids], level_T) if bank is not None else [(0, 0)] * len(vids)
        records = [bank.get(der.clip_key(v))[0] if r[0] else None for v, r in zip(vids, rows)]
        return der.der_term(logits, level_row, level_T, level_len, records, self.der_alpha)[0]

    def _pod_loss(self, fpn_feats, level_len):
        """cl_name 'pod' (ours; cl_methods/pod.py): PODNet's pooled feature distillation of the step's pyramid against the records
        the incoming model left for the batch's clips, times pod_lambda * sqrt(n_classes / new classes) (host arithmetic).  On
        the device ONE ops.pod_distill call (csrc/pod.hip) over the level list, the records named by a device table; a CPU model
        evaluates the same term in tensor ops."""
        from ..cl_methods import pod
        (tab, video_list), self._pod_tab_step = getattr(self, "_pod_tab_step", None) or (None, None), None
        if fpn_feats is None:
            raise ValueError("a cl_name 'pod' step needs the pyramid features of the step")
        fpn_feats = list(fpn_feats)
        level_T, Cn = tuple(int(f.shape[1]) for f in fpn_feats), int(fpn_feats[0].shape[2])
        scale = pod.adaptive_scale(self.pod_lambda, self.cls_head.cls_head.conv.out_channels, self.n_known)
        if fpn_feats[0].is_cuda:
            if tab is None:
                if video_list is None:
                    raise ValueError("a cl_name 'pod' step needs StepInputs.pod_tab or the list of its clips")
                tab = pod.step_table(self, video_list, level_T)
            return ops.pod_distill(fpn_feats, level_len, tab, scale)
        if video_list is None:
            raise ValueError("a cl_name 'pod' step on a CPU model needs the list of its clips")
        vids, bank = pod.labelled(video_list), self.pod_bank
        rows = bank.rows_for(vids, [pod.clip_len(v) for v in vids], level_T, Cn) if bank is not None else [0] * len(vids)
        records = [bank.get(pod.clip_key(v))[0] if r else None for v, r in zip(vids, rows)]
        return pod.pod_term(fpn_feats, level_len, records, scale)[0]

    def _erd_loss(self, out_cls_logits, cat_logits, cat_offsets, level_len):
        """cl_name 'erd' (ours; cl_methods/erd.py): at the positions the incoming model answered confidently on the batch's clips,
        the squared distance of the logits over the classes known then and the DIoU of the offsets against the records.  On the
        device ONE ops.erd_distill call (csrc/erd.hip) over the concatenated head output -- the fused loss route hands it the raw
        offsets and the per-level Scale --, the records named by a device table; a CPU model evaluates the same term in tensor
        ops.  -> (erd_loss, its classification part, its regression part)"""
        from ..cl_methods import erd
        (tab, video_list), self._erd_tab_step = getattr(self, "_erd_tab_step", None) or (None, None), None
        if cat_offsets is None:
            raise ValueError("a cl_name 'erd' step needs the offsets of the step")
        (logits, level_row), (offsets, scale) = cat_logits, cat_offsets
        level_T = tuple(int(x.shape[1]) for x in out_cls_logits)
        if logits.is_cuda:
            if tab is None:
                if video_list is None:
                    raise ValueError("a cl_name 'erd' step needs StepInputs.erd_tab or the list of its clips")
                tab = erd.step_table(self, video_list, level_T)
            return ops.erd_distill(logits, offsets, scale, level_row, level_T, level_len, tab, self.erd_lambda_cls,
                                   self.erd_lambda_reg)
        if video_list is None:
            raise ValueError("a cl_name 'erd' step on a CPU model needs the list of its clips")
        vids, bank = erd.labelled(video_list), self.erd_bank
        records = (bank.usable(vids, [erd.clip_len(v) for v in vids], level_T) if bank is not None else [None] * len(vids))
        return erd.erd_term(logits, offsets, scale, level_row, level_T, level_len, records, self.erd_lambda_cls,
                            self.erd_lambda_reg)[:3]

    def _cl_terms(self, out, final_loss, out_cls_logits, prev_out_cls_logits, reduce_sim, cat_logits=None, level_len=None,
                  fpn_feats=None, cat_offsets=None):
        """continual-learning terms on top of the detection loss (meta_archs.py:1478-1519).  On the device the iCaRL / BiC
        distillation term is one fused op (cat_logits = the concatenated logits and every level's first row in them); a
        CPU model walks the reference's loops.  level_len: int32 [B, L] valid lengths, read by the 'der' term only."""
        if self.n_known > 0 and self.cl_name == 'l2p' and reduce_sim is not None:      # (a CODA-Prompt pool has no pull term)
            final_loss = final_loss - 0.1 * reduce_sim
        coda_ortho = getattr(self, '_coda_ortho', None)             # set by forward_prepared on a model with a CodaPrompt
        if coda_ortho is not None and self.coda_ortho_mu != 0.0:
            out['ortho_loss'] = self.coda_ortho_mu * coda_ortho
            final_loss = final_loss + out['ortho_loss']
        if self.n_known > 0 and self.cl_name == 'der':
            der_loss = self._der_loss(out_cls_logits, cat_logits, level_len)
            out['der_loss'] = der_loss
            out['final_loss'] = final_loss + der_loss
            return out
        if self.n_known > 0 and self.cl_name == 'pod':      # fpn_feats: the pyramid of the step, level_len as for 'der'
            pod_loss = self._pod_loss(fpn_feats, level_len)
            out['pod_loss'] = pod_loss
            out['final_loss'] = final_loss + pod_loss
            return out
        if self.n_known > 0 and self.cl_name == 'erd':      # cat_offsets: the offsets in the logits' rows and the Scale, or None
            erd_loss, erd_cls, erd_reg = self._erd_loss(out_cls_logits, cat_logits, cat_offsets, level_len)
            out['erd_loss'], out['erd_cls_loss'], out['erd_reg_loss'] = erd_loss, erd_cls.detach(), erd_reg.detach()
            out['final_loss'] = final_loss + erd_loss
            return out
        if self.n_known > 0 and self.cl_name in ('bic', 'icarl') and out_cls_logits[0].is_cuda:
            dist_loss = self._device_distill(out_cls_logits, prev_out_cls_logits, cat_logits)
            out['dist_loss'] = dist_loss
            out['final_loss'] = final_loss + dist_loss
            return out
        if self.n_known > 0 and self.cl_name == 'bic':
            n_classes = self.cls_head.cls_head.conv.out_channels
            alpha, temp, dist_loss = self.n_known / n_classes, 2, 0
            for cur, prev in zip(out_cls_logits, prev_out_cls_logits):
                prev = _as_device(prev, cur.device)
                logp = F.log_softmax(cur[0, :, :self.n_known] / temp, dim=1)
                dist_loss = dist_loss + 0.01 * alpha * -torch.mean(torch.sum(prev[:, :self.n_known] * logp, dim=1))
            final_loss = final_loss + dist_loss
            out['dist_loss'] = dist_loss
        if self.n_known > 0 and self.cl_name == 'icarl':
            len_f, dist_loss = len(out_cls_logits), 0
            for i in range(len_f):
                if len(prev_out_cls_logits) != len_f or len(prev_out_cls_logits) == 1:
                    prev_out_cls_logits = prev_out_cls_logits[0]
                prev = _as_device(prev_out_cls_logits[i], out_cls_logits[i].device)
                dist_loss = dist_loss + 0.01 * sum(self.dist_loss(out_cls_logits[i][0, :, y], prev[:, y])
                                                   for y in range(self.n_known))
            final_loss = final_loss + dist_loss
            out['dist_loss'] = dist_loss
        out['final_loss'] = final_loss
        return out

    # ------------------------------------------------------------------ iCaRL nearest-exemplar-mean classification
    @torch.no_grad()
    def _pyramid_features(self, video_list):
        """backbone + neck of an inference batch (one clip): list over levels of token-major [1, T_l, C].
        The text goes in RAW: the reference's classify hands query_preprocessing's tokens and mask straight to the backbone
        (meta_archs.py:1077-1079, 1108-1110), also on a model with an L2P prompt pool."""
        inp = self.prepare(video_list, is_training=False)
        x_tm = ops.transpose(inp.feats_cf)
        text_tm = text_lens = None
        if self.use_cross_modal:
            text_tm, text_lens = ops.transpose(inp.text_cf), inp.text_lens
        feats, all_lens = self.backbone.forward_tm(x_tm, inp.lens, text_tm, text_lens)
        return self.neck.forward_tm(feats, all_lens)[0]

    @torch.no_grad()
    def classify(self, x, cilsettask):
        """iCaRL's classifier (meta_archs.py:1061-1131): squared distances between the clip's normalised pyramid features
        and the class means of the exemplars in `self.memory` -> list over levels of [1, T_l, n_classes].
        The means are (re)computed while `compute_means` is set (`cilsettask.get_dataloader({class: clips},
        sample_frame=True)` yields the exemplars as one-clip batches): each exemplar's level-l map is divided by its
        Frobenius norm, the maps are averaged per class and normalised again.
        One difference: the reference hard-codes `fpn_levels = 10` (:1065) and therefore fails on any other pyramid
        depth (the shipped (2, 2, 5) architectures have 6 levels); the level count is taken from the model here.  On a
        10-level model the outputs equal the reference's (tests/test_icarl.py)."""
        if self.compute_means:
            means = None
            for class_id, videos in self.memory.items():
                per_level = None
                for video_list in cilsettask.get_dataloader({class_id: videos}, sample_frame=True):
                    f = [t / t.norm() for t in self._pyramid_features(video_list)]
                    per_level = [[a] for a in f] if per_level is None else [l + [a] for l, a in zip(per_level, f)]
                mus = []
                for lvl in per_level:
                    mu = torch.stack(lvl, dim=0).mean(0)[0]               # [T_l, C]
                    mus.append(mu / mu.norm())
                means = [[m] for m in mus] if means is None else [l + [m] for l, m in zip(means, mus)]
            self.exemplar_means = [torch.stack(l, dim=0) for l in means]          # per level [n_classes, T_l, C]
            self.compute_means = False
        dists = []
        for f, m in zip(self._pyramid_features([x]), self.exemplar_means):
            fn = f / f.norm()                                                      # [1, T_l, C]
            dists.append((fn.unsqueeze(1) - m.unsqueeze(0)).pow(2).sum(-1).permute(0, 2, 1).contiguous())   # [1, T_l, n_cls]
        return dists

    # ------------------------------------------------------------------ inference
    @torch.no_grad()
    def inference(self, video_list, points, fpn_masks, out_cls_logits, out_offsets, out_lb_logits,
                  out_rb_logits, cilsettask=None):
        results = []
        for idx, vl in enumerate(video_list):
            # final validation of an iCaRL run (meta_archs.py:1561-1562): class distances of this clip.  `classify`
            # clears compute_means once the exemplar means exist, so -- as in the reference -- only the first clip
            # validated after training is decoded from distances; the following ones take the ordinary path.
            cls_preds = self.classify(vl, cilsettask) if (cilsettask is not None and self.compute_means) else None
            r = self.inference_single_video(points, [x[idx] for x in fpn_masks],
                                            [x[idx] for x in out_cls_logits], [x[idx] for x in out_offsets],
                                            None, None, cls_preds_per_vid=cls_preds)
            for k_out, k_in in (('video_id', 'video_id'), ('fps', 'fps'), ('duration', 'duration'),
                                ('feat_stride', 'feat_stride'), ('feat_num_frames', 'feat_num_frames')):
                r[k_out] = vl[k_in]
            results.append(r)
        return self.postprocessing(results)

    @torch.no_grad()
    def inference_single_video(self, points, fpn_masks, out_cls_logits, out_offsets, lb_logits_per_vid=None,
                               rb_logits_per_vid=None, candidate_label=None, cls_preds_per_vid=None):
        """threshold -> top-k -> decode per level (meta_archs.py:1594-1692).  On the device the whole pyramid of the clip
        is one vilco_decode call (exact top-k by radix select, one host read: the candidate count); VILCO_DEVICE_DECODE=0
        or host tensors take the tensor-expression path below, which mirrors the reference line by line."""
        if cls_preds_per_vid is None and out_cls_logits[0].is_cuda and switches.on("VILCO_DEVICE_DECODE"):
            lens = [int(c.shape[0]) for c in out_cls_logits]
            row0 = torch.tensor([sum(lens[:i]) for i in range(len(lens))], dtype=torch.int32, device=out_cls_logits[0].device)
            level_len = torch.stack([m.sum() for m in fpn_masks]).to(torch.int32)
            segs, scores, labels = ops.decode(torch.cat(out_cls_logits).float().contiguous(), torch.cat(out_offsets).float().contiguous(),
                                              torch.cat(points).float().contiguous(), row0, level_len, self.test_pre_nms_topk,
                                              self.test_pre_nms_thresh, self.test_duration_thresh)
            return {'segments': segs, 'scores': scores, 'labels': labels}
        segs_all, scores_all, cls_all = [], [], []
        for lvl, (cls_i, off_i, pts_i, mask_i) in enumerate(zip(out_cls_logits, out_offsets, points, fpn_masks)):
            prob = (cls_i.sigmoid() * mask_i.unsqueeze(-1)).flatten()
            if cls_preds_per_vid is not None:
                # iCaRL (meta_archs.py:1626-1643): candidates = (position, class) pairs closer to their class mean than the
                # level's average distance, ranked by distance.  The rank indices address the unfiltered distance array
                # but are applied to the filtered candidates; when they would run past the end every candidate is kept.
                dist = cls_preds_per_vid[lvl].flatten()
                keep = dist < dist.mean()
                prob = prob[keep]
                topk_idxs = keep.nonzero(as_tuple=True)[0]
                num_topk = min(self.test_pre_nms_topk, topk_idxs.size(0))
                order = dist.sort(descending=False)[1]
                if not bool(order[:num_topk].max() > prob.shape[0]):
                    prob = prob[order[:num_topk]].clone()
                    topk_idxs = topk_idxs[order[:num_topk]].clone()
            else:
                keep = prob > self.test_pre_nms_thresh
                prob = prob[keep]
                topk_idxs = keep.nonzero(as_tuple=True)[0]
                num_topk = min(self.test_pre_nms_topk, topk_idxs.size(0))
                prob, order = prob.sort(descending=True)
                prob = prob[:num_topk].clone()
                topk_idxs = topk_idxs[order[:num_topk]].clone()
            pt_idxs = torch.div(topk_idxs, self.num_classes, rounding_mode='floor')
            cls_idxs = torch.fmod(topk_idxs, self.num_classes)
            offs, pts = off_i[pt_idxs], pts_i[pt_idxs]
            left = pts[:, 0] - offs[:, 0] * pts[:, 3]
            right = pts[:, 0] + offs[:, 1] * pts[:, 3]
            keep2 = (right - left) > self.test_duration_thresh
            segs_all.append(torch.stack((left, right), -1)[keep2])
            scores_all.append(prob[keep2])
            cls_all.append(cls_idxs[keep2])
        return {'segments': torch.cat(segs_all), 'scores': torch.cat(scores_all), 'labels': torch.cat(cls_all)}

    @torch.no_grad()
    def postprocessing(self, results):
        """device NMS, then seconds conversion and the single D2H copy (meta_archs.py:1695-1736)."""
        out = []
        for r in results:
            segs, scores, labels = r['segments'].detach(), r['scores'].detach(), r['labels'].detach()
            if self.test_nms_method != 'none':
                segs, scores, labels = batched_nms(segs, scores, labels, self.test_iou_threshold,
                                                   self.test_min_score, self.test_max_seg_num,
                                                   use_soft_nms=(self.test_nms_method == 'soft'),
                                                   multiclass=self.test_multiclass_nms, sigma=self.test_nms_sigma,
                                                   voting_thresh=self.test_voting_thresh)
            if segs.shape[0] > 0:
                segs = (segs * r['feat_stride'] + 0.5 * r['feat_num_frames']) / r['fps']
                segs = torch.where(segs <= 0.0, segs * 0.0, segs)
                vlen = r['duration']
                segs = torch.where(segs >= vlen, segs * 0.0 + vlen, segs)
            out.append({'video_id': r['video_id'], 'segments': segs.cpu(), 'scores': scores.cpu(),
                        'labels': labels.cpu()})
        return out

    # ------------------------------------------------------------------ replay memory (train_cl.py:343-361)
    def add_samples_to_mem(self, cilsettask, data, m):
        """random replay-memory sampling: merge the episode's {class: videos} into the memory, shuffle
        each class in place and keep m per class ('ALL' keeps everything) (meta_archs.py:1046-1052)."""
        if self.type_sampling == 'herding':
            return self._herd_samples_to_mem(cilsettask, data, m)
        import random
        self.memory = {**self.memory, **data}
        for class_id, videos in self.memory.items():
            random.shuffle(videos)
            self.memory[class_id] = videos[:m] if m != 'ALL' else videos
        for class_id, videos in self.memory.items():
            print('Memory... Class: {}, num videos: {}'.format(class_id, len(videos)))

    @torch.no_grad()
    def herding_order(self, cilsettask, class_id, videos, m):
        """iCaRL's herding over the candidates of one class -> (clips in loader order, device int32 [min(m, N)] of the
        selected positions, in selection order).  The descriptor of a clip is what `classify` averages: every level map
        of `_pyramid_features` (eval mode) divided by its Frobenius norm.  Greedy step: the clip whose addition brings the
        normalised sum of the selected descriptors closest to the normalised class mean, summed over the levels; ties go
        to the earlier clip.  The reference's own branch (meta_archs.py:973-1043) is commented out and unfinished; the
        definition is spelled out in include/vilco_hip.h and DESIGN.md 3.10.
        The level maps go into one preallocated [N, T_l * C] buffer per level; vilco_frob_scale, vilco_gram (the row scale
        folded into the product) and vilco_herd_select do the rest, the indices stay on the device."""
        batches = list(cilsettask.get_dataloader({class_id: videos}, sample_frame=True))
        for b in batches:
            if len(b) != 1:
                raise ValueError("herding needs one-clip batches, got a batch of %d for class %r" % (len(b), class_id))
        N = len(batches)
        dev = next(self.parameters()).device
        if N == 0:
            return [], torch.empty(0, dtype=torch.int32, device=dev)
        was_training = self.training
        self.eval()
        try:
            bufs, shapes = None, None
            for i, vl in enumerate(batches):
                f = self._pyramid_features(vl)
                if bufs is None:
                    shapes = [tuple(t.shape) for t in f]
                    need = 4 * N * sum(t.numel() for t in f)
                    free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
                    if need > free:
                        raise RuntimeError("herding class %r: the descriptors of its %d clips need %d bytes, %d bytes of "
                                           "device memory are free" % (class_id, N, need, free))
                    bufs = [torch.empty(N, t.numel(), dtype=torch.float32, device=dev) for t in f]
                elif [tuple(t.shape) for t in f] != shapes:
                    raise ValueError("herding class %r: clip %r has level shapes %s, the class's first clip %s"
                                     % (class_id, vl[0].get('video_id', i), [tuple(t.shape) for t in f], shapes))
                for buf, t in zip(bufs, f):
                    buf[i].copy_(t.reshape(-1))
        finally:
            self.train(was_training)
        grams = torch.stack([ops.gram(buf, ops.frob_scale(buf), torch.float64) for buf in bufs], dim=0)
        return [b[0] for b in batches], ops.herd_select(grams, N if m == 'ALL' else m)

    def _herd_samples_to_mem(self, cilsettask, data, m):
        """type_sampling 'herding' (beyond the reference, which samples at random whatever the setting): every class of
        `data` becomes its clips in herding order, a priority list, so a class already in memory shrinks by videos[:m]
        without reshuffling (what meta_archs.py:1043 intended).  m == 'ALL' keeps every clip, still in herding order."""
        if cilsettask is None:
            raise ValueError("type_sampling 'herding' needs the task stream (get_dataloader) to compute the descriptors")
        memory = {**self.memory, **data}
        for class_id, videos in memory.items():
            if class_id in data:
                clips, sel = self.herding_order(cilsettask, class_id, videos, m)
                memory[class_id] = [clips[i] for i in sel.tolist()]
            else:
                memory[class_id] = videos[:m] if m != 'ALL' else videos
        self.memory = memory
        for class_id, videos in self.memory.items():
            print('Memory... Class: {}, num videos: {}'.format(class_id, len(videos)))
