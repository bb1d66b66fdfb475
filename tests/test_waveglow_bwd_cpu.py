"""CPU checks for WaveGlow training: the float64 restatement of the backward pass (tests/_waveglow_bwd_ref.py) against
the reference's recorded gradients (tests/golden/waveglow_bwd_tiny.npz), and the weight-norm parameters of
rad_mmm_amd.waveglow.WaveGlow (module construction needs no GPU)."""
import numpy as np
import torch

from _waveglow_bwd_ref import grads_ref, rel_l2
from _waveglow_ref import HOP, load_fixture


def test_restatement_reproduces_the_reference_gradients(golden):
    # float32 storage of two float64 computations: 1e-6 relative L2
    fwd, bwd = golden("waveglow_fwd_tiny.npz"), golden("waveglow_bwd_tiny.npz")
    cfg, sd = load_fixture(fwd)
    n = int(fwd["eq_T"])
    mel, audio = torch.from_numpy(fwd["mel"][:, :, :n].copy()), torch.from_numpy(fwd["audio"][:, :n * HOP].copy())
    loss, grads = grads_ref(sd, cfg, mel, audio, [n, n])
    assert abs(loss - float(bwd["loss64"])) <= 1e-12
    names = [k[5:] for k in bwd if k.startswith("grad/")]
    assert len(names) >= 100 and "upsample.weight" in names and "WN.2.cond_layer.weight_v" in names
    worst = 0.0
    for k in names:
        err = rel_l2(grads[k].numpy(), bwd["grad/" + k])
        worst = max(worst, err)
        assert err <= 1e-6, (k, err)
    print(f"{len(names)} gradients, worst relative L2 {worst:.3e}")


def test_weight_norm_round_trip(golden):
    from rad_mmm_amd.waveglow import WaveGlow, fold_weight_norm_keys
    cfg, sd = load_fixture(golden("waveglow_fwd_tiny.npz"))
    m = WaveGlow(**cfg)
    folded_keys = set(m.state_dict())
    assert m.apply_weight_norm() is m
    got = m.state_dict()
    assert set(got) == set(sd) and all(got[k].shape == sd[k].shape for k in sd)
    assert set(n for n, _ in m.named_parameters()) == set(sd)
    m.load_state_dict(sd)                                  # unfolded, as it stands
    assert all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)
    m.remove_weight_norm()
    want = fold_weight_norm_keys(sd)
    got = m.state_dict()
    assert set(got) == set(want) == folded_keys and all(torch.equal(got[k], want[k]) for k in want)
    m.apply_weight_norm()                                  # g = the rows' norms, v = the weight
    sd2 = m.state_dict()
    for k, w in want.items():
        if k[:-len(".weight")] + ".weight_g" in sd2:
            v, g = sd2[k[:-len("weight")] + "weight_v"], sd2[k[:-len("weight")] + "weight_g"]
            back = v * (g / v.reshape(v.shape[0], -1).norm(dim=1).reshape(-1, 1, 1))
            assert float((back - w).norm() / w.norm()) <= 1e-7, k
    m.load_state_dict(want)                                # a folded dict into the weight-normed form
    m.remove_weight_norm()
    assert all(float((m.state_dict()[k] - want[k]).norm() / want[k].norm()) <= 1e-7 for k in want if want[k].dim() == 3)
    assert not any("weight_g" in k for k in m.state_dict())
