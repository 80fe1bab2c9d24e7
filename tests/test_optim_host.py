"""Host side of the native optimiser (rohm_amd/optim.py) and of its switches in the loops and the driver; no GPU."""
import types

import pytest
import torch

from rohm_amd import optim
from rohm_amd.train import TrainLoopPoseNet
from rohm_amd.train.__main__ import parse_args


def _p(dtype=torch.float32):
    return torch.zeros(3, dtype=dtype, requires_grad=True)


@pytest.mark.parametrize('option', ['amsgrad', 'maximize', 'capturable', 'differentiable'])
def test_constructor_refuses_the_variants(option):
    with pytest.raises(ValueError, match=option):
        optim.AdamW([_p()], **{option: True})


def test_constructor_refuses_cpu_and_non_fp32_parameters():
    with pytest.raises(ValueError, match='HIP device'):
        optim.AdamW([_p()])
    with pytest.raises(ValueError, match='fp32'):
        optim.AdamW([_p(torch.float64)])
    with pytest.raises(ValueError, match='fp32'):
        optim.AdamW([{'params': [_p(torch.bfloat16)], 'lr': 1e-3}])
    with pytest.raises(ValueError, match='beta'):
        optim.AdamW([_p()], betas=(0.3, 0.999))
    with pytest.raises(ValueError, match='max_grad_norm'):
        optim.AdamW([_p()], max_grad_norm=-1.0)


def test_state_dict_layout_is_torchs(monkeypatch):
    """Same groups, same keys: param_groups option for option, and the per-parameter state entries with torch's types.  The
    device check is lifted for this test alone: the layout is host logic."""
    monkeypatch.setattr(optim.AdamW, '_check_param', staticmethod(lambda p: None))
    groups = lambda: [dict(params=[_p(), _p()], lr=1e-3, weight_decay=0.0),      # noqa: E731
                      dict(params=[_p()], lr=3e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.01)]
    ref = torch.optim.AdamW(groups())
    own = optim.AdamW(groups(), max_grad_norm=1.0)
    assert own.state_dict() == ref.state_dict()                   # no state yet: the groups alone
    for g in ref.param_groups:
        for p in g['params']:
            p.grad = torch.ones_like(p)
    ref.step()
    for g in own.param_groups:
        for p in g['params']:
            own._state_of(p)['step'] += 1
    a, b = own.state_dict(), ref.state_dict()
    assert a['param_groups'] == b['param_groups'] and set(a) == set(b)
    assert sorted(a['state']) == sorted(b['state']) == [0, 1, 2]
    for k in a['state']:
        assert list(a['state'][k]) == list(b['state'][k]) == ['step', 'exp_avg', 'exp_avg_sq']
        for name in a['state'][k]:
            x, y = a['state'][k][name], b['state'][k][name]
            assert (x.dtype, x.device, x.shape) == (y.dtype, y.device, y.shape), name
        assert float(a['state'][k]['step']) == float(b['state'][k]['step']) == 1.0
    # and each loads into the other
    torch.optim.AdamW(groups()).load_state_dict(a)
    optim.AdamW(groups()).load_state_dict(b)


def test_driver_arguments(tmp_path):
    for which in ('posenet', 'trajnet'):
        d = parse_args(which, [])
        assert d.optimizer == 'torch' and d.max_grad_norm is None
        c = parse_args(which, ['--optimizer', 'native', '--max_grad_norm', '1.5'])
        assert c.optimizer == 'native' and c.max_grad_norm == 1.5 and isinstance(c.max_grad_norm, float)
    cfg = tmp_path / 'cfg.yaml'
    cfg.write_text('optimizer: native  # the fused step\nmax_grad_norm: 0.5\nlr: 1e-4\n')
    a = parse_args('posenet', ['--config', str(cfg)])
    assert a.optimizer == 'native' and a.max_grad_norm == 0.5 and a.lr == 1e-4
    a = parse_args('posenet', ['--config', str(cfg), '--max_grad_norm', '2'])
    assert a.max_grad_norm == 2.0
    cfg.write_text('optimizer: native\nmax_grad_norm: None\n')      # what the driver's own config.yaml dump holds
    assert parse_args('trajnet', ['--config', str(cfg)]).max_grad_norm is None
    cfg.write_text('optimizer: sgd\n')
    with pytest.raises(ValueError, match='optimizer must be one of'):
        parse_args('posenet', ['--config', str(cfg)])
    with pytest.raises(SystemExit):
        parse_args('posenet', ['--optimizer', 'sgd'])


def test_max_grad_norm_with_the_torch_optimiser_is_refused(tmp_path):
    with pytest.raises(ValueError, match='max_grad_norm needs optimizer'):
        parse_args('posenet', ['--max_grad_norm', '1.0'])
    cfg = tmp_path / 'cfg.yaml'
    cfg.write_text('max_grad_norm: 1.0\n')
    with pytest.raises(ValueError, match='max_grad_norm needs optimizer'):
        parse_args('trajnet', ['--config', str(cfg)])

    class Loader:
        dataset = types.SimpleNamespace(clip_len=16, traj_feat_dim=22)

        def __len__(self):
            return 1

    def loop(**extra):
        args = types.SimpleNamespace(batch_size=2, lr=1e-3, log_interval=10, save_interval=10, weight_decay=0.0, num_steps=1,
                                     dataset_root='/nowhere/AMASS', **extra)
        return TrainLoopPoseNet(args, writer=None, model=torch.nn.Linear(2, 2), diffusion_train=types.SimpleNamespace(num_timesteps=4),
                                diffusion_eval=None, timestep_respacing_eval='', input_noise=True, train_dataloader=Loader(),
                                test_dataloader=None, logdir=str(tmp_path), logger=None, start_prox_mask_epoch=10,
                                mask_scheme='lower', device='cpu')
    assert type(loop().opt) is torch.optim.AdamW
    assert type(loop(optimizer='torch').opt) is torch.optim.AdamW
    with pytest.raises(ValueError, match="max_grad_norm needs optimizer='native'"):
        loop(max_grad_norm=1.0)
    with pytest.raises(ValueError, match="max_grad_norm needs optimizer='native'"):
        loop(optimizer='torch', max_grad_norm=1.0)
    with pytest.raises(ValueError, match="must be 'torch' or 'native'"):
        loop(optimizer='sgd')
    with pytest.raises(ValueError, match='HIP device'):
        loop(optimizer='native')                              # a CPU model: the native optimiser has no CPU fallback
