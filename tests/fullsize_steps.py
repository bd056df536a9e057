"""The three training steps whose every kernel call the full-size census tests check (test infrastructure):

  "P"    -- bench.py's headline workload: config P (T = 2304, Cin = 2304, D = 1024, H = 16, XLNet layer) in train mode
            with dropout / droppath / XLNet dropout 0.1, single-part weight-gradient products on;
  "W"    -- bench.side_config("W"): config P with D = 2304 (hd = 144), no XLNet layer, droppath 0.1;
  "cfg1" -- bench.side_config("cfg1"): BASELINE configs[0] (T = 256, Cin = 512, D = 512, H = 4, XLNet hd = 128), droppath 0.1.

The configuration dicts restate bench.side_config's (which builds and times its model in one go)."""
import torch

STEPS = ("P", "W", "cfg1")


def build_step(name, dev):
    """(model, batch) of one step; the model in train mode, seeded like bench.py"""
    import bench
    import vilco_amd.modeling as vm
    from vilco_amd.core.config import make_config
    if name == "P":
        cfg = bench.p_config()
        torch.manual_seed(0)
        model = vm.make_meta_arch('LocPointTransformer', **dict(cfg, xlnet_config=bench.p_xlnet())).to(dev).train()
        return model, bench.synth_batch(2, dev)
    if name == "W":
        over = dict(dataset=dict(input_dim=2304, num_classes=22, max_seq_len=2304),
                    model=dict(embd_dim=2304, fpn_dim=2304, head_dim=2304, n_head=16, backbone_arch=(2, 2, 5), use_abs_pe=True,
                               use_cross_modal=True, n_txt_in=768, max_buffer_len_factor=1.0, use_xl=False),
                    train_cfg=dict(init_loss_norm=100, dropout=0.0, droppath=0.1))
        T, Cin, xl = 2304, 2304, None
    elif name == "cfg1":
        over = dict(dataset=dict(input_dim=512, num_classes=22, max_seq_len=256),
                    model=dict(embd_dim=512, fpn_dim=512, head_dim=512, n_head=4, backbone_arch=(2, 2, 5), use_abs_pe=True,
                               use_cross_modal=True, n_txt_in=768, max_buffer_len_factor=1.0, use_xl=True),
                    train_cfg=dict(init_loss_norm=100, dropout=0.0, droppath=0.1))
        T, Cin = 256, 512
        xl = dict(bench.P_XLNET, d_model=512, n_head=4, d_head=128, d_inner=1024, dropout=0.0)
    else:
        raise ValueError(name)
    cfg = make_config(**over)['model']
    torch.manual_seed(0)
    kw = dict(cfg, xlnet_config=xl) if xl is not None else dict(cfg)
    model = vm.make_meta_arch('LocPointTransformer', **kw).to(dev).train()
    return model, bench.synth_batch(2, dev, seed=0, T=T, Cin=Cin)


def run_step(model, batch):
    """one eager forward + backward; returns the losses as floats"""
    model.zero_grad(set_to_none=True)
    out = model(batch, is_training=True)
    out['final_loss'].backward()
    torch.cuda.synchronize()
    return {k: float(v.detach()) for k, v in out.items()}
