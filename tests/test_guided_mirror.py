"""decoder.FeatureGuidedSAAG against the reference's own class (tests/golden/FG1_guided_mods.npz, written by
tests/golden/make_goldens_guided.py), and the command line of --experiment 3 --decoder guided_saag.  No GPU.

TOL = 1e-6 in the project's form, of the tensor's largest magnitude (helpers.rel_to_max): the fixture's gradients reach 3.9, where
one fp32 ulp is 2.4e-7 and the 70-term sums of the two linear layers are added in an order that differs between CPUs (the same
fp32 run is 1.7e-6 = 7 ulps away in absolute terms on another host, 4e-7 of the largest magnitude)."""
import os

import numpy as np
import pytest
import torch

from helpers import rel_to_max

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "FG1_guided_mods.npz")
KEYS = ("aspect_ratio_mult", "edge_threshold_add", "edge_shrink_mult", "normal_strength_mult", "base_size_mult", "opacity_mult")
TOL = 1e-6


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("tag, dtype", [("f32", torch.float32), ("f64", torch.float64)])
def test_mirror_matches_the_reference(golden, tag, dtype):
    from fresnel_amd.decoder import FeatureGuidedSAAG
    from fresnel_amd.surface import MOD_KEYS
    assert tuple(golden["keys"]) == KEYS == MOD_KEYS
    state = {k[len("state."):]: torch.from_numpy(golden[k]) for k in golden.files if k.startswith("state.")}
    assert sorted(state) == ["net.0.bias", "net.0.weight", "net.2.bias", "net.2.weight"]
    assert float(np.abs(golden["state.net.2.weight"]).min()) > 0.0           # the fixture's last layer is not the zero init
    model = FeatureGuidedSAAG(feature_dim=8, num_params=6, hidden_dim=4)
    assert list(model.state_dict()) == ["net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias"]
    model.load_state_dict(state, strict=True)
    model = model.to(dtype)
    maps = model(torch.from_numpy(golden["features"]).to(dtype))
    assert tuple(maps) == KEYS
    weights = torch.from_numpy(golden["weights"]).to(dtype)
    sum((weights[i] * maps[k]).sum() for i, k in enumerate(KEYS)).backward()
    for k in KEYS:
        want = golden[f"{tag}.map.{k}"]
        assert maps[k].shape == (2, 5, 7) and maps[k].dtype == dtype
        assert rel_to_max(maps[k].detach().numpy(), want) <= TOL, k
    for name, p in model.named_parameters():
        want = golden[f"{tag}.grad.{name}"]
        assert np.abs(want).max() > 1e-3
        assert rel_to_max(p.grad.numpy(), want) <= TOL, name


def test_defaults_and_zero_initialised_last_layer():
    """The reference's constructor defaults; an untrained model predicts the identity (1, 0, 1, 1, 1, 1): the plain SAAG cloud."""
    from fresnel_amd.decoder import FeatureGuidedSAAG
    model = FeatureGuidedSAAG()
    assert (model.feature_dim, model.num_params) == (384, 6)
    assert model.net[0].in_features == 384 and model.net[0].out_features == 64 and model.net[2].out_features == 6
    assert not model.net[2].weight.any() and not model.net[2].bias.any()
    maps = model(torch.randn(2, 384, 3, 4))
    for k, want in zip(KEYS, (1.0, 0.0, 1.0, 1.0, 1.0, 1.0)):
        assert maps[k].shape == (2, 3, 4) and bool((maps[k] == want).all()), k


def test_maps_stack_in_channel_order():
    from fresnel_amd import _binding as B
    from fresnel_amd.surface import mods_tensor
    maps = {k: torch.full((2, 3, 4), float(i)) for i, k in enumerate(KEYS)}
    t = mods_tensor(dict(reversed(list(maps.items()))))                  # the dict's own order does not matter
    assert t.shape == (2, 6, 3, 4) and all(bool((t[:, i] == i).all()) for i in range(6))
    assert mods_tensor(t) is t
    with pytest.raises(B.FgsError):
        mods_tensor({k: maps[k] for k in KEYS[:5]})
    with pytest.raises(B.FgsError):
        mods_tensor(torch.zeros(2, 5, 3, 4))


def test_command_line_of_experiment_3():
    from fresnel_amd import train
    from fresnel_amd.decoder import FeatureGuidedSAAG
    ap = train.arg_parser()
    with pytest.raises(SystemExit, match="guided_saag"):                 # bare: refused, and the message names the accepted spelling
        train.config_from_args(ap.parse_args(["--experiment", "3"]))
    with pytest.raises(SystemExit):
        train.main(["--experiment", "3"])
    cfg = train.config_from_args(ap.parse_args(["--experiment", "3", "--decoder", "guided_saag"]))
    assert (cfg.experiment, cfg.decoder, cfg.surface_subsample) == (3, "guided_saag", 4)
    cfg = train.config_from_args(ap.parse_args(["--experiment", "3", "--decoder", "guided_saag", "--surface_subsample", "2"]))
    assert cfg.surface_subsample == 2
    cfg.feature_dim = 8
    model = train.make_decoder(cfg)
    assert isinstance(model, FeatureGuidedSAAG) and model.net[0].in_features == 8 and model.net[0].out_features == 64
    for bad in (["--decoder", "guided_saag"], ["--experiment", "2", "--decoder", "guided_saag"],
                ["--experiment", "1", "--decoder", "guided_saag"], ["--experiment", "3", "--decoder", "saag"],
                ["--experiment", "3", "--decoder", "direct"], ["--experiment", "3", "--decoder", "guided_saag", "--hip_graph"],
                ["--experiment", "3", "--decoder", "guided_saag", "--stochastic_k", "100"],
                ["--experiment", "3", "--decoder", "guided_saag", "--fast_mode"],
                ["--experiment", "3", "--decoder", "guided_saag", "--surface_subsample", "0"]):
        with pytest.raises(SystemExit):
            train.config_from_args(ap.parse_args(bad))


def test_run_training_refuses_a_cpu_device_and_a_graph():
    from fresnel_amd import train
    ap = train.arg_parser()
    cfg = train.config_from_args(ap.parse_args(["--experiment", "3", "--decoder", "guided_saag"]))
    cfg.device = "cpu"
    with pytest.raises(ValueError, match="GPU"):
        train.run_training(cfg, log=lambda *a: None)
    cfg.device, cfg.hip_graph = "cuda:0", True
    with pytest.raises(ValueError, match="hip_graph"):
        train.run_training(cfg, log=lambda *a: None)


def test_file_names_follow_exp3(tmp_path):
    from fresnel_amd import train
    cfg = train.config_from_args(train.arg_parser().parse_args(["--experiment", "3", "--decoder", "guided_saag", "--output_dir", str(tmp_path)]))
    assert train.save_training_history({"total": [1.0]}, cfg).name == "training_history_exp3.json"


def test_surface_command_line_takes_a_guide(tmp_path):
    """--guide loads an experiment-3 checkpoint strictly and hands the generator the maps of the batch's features."""
    from fresnel_amd import surface
    from fresnel_amd.decoder import FeatureGuidedSAAG
    assert surface.build_parser().parse_args(["--data_dir", "x"]).guide is None
    model = FeatureGuidedSAAG(feature_dim=8, hidden_dim=4)
    with torch.no_grad():
        model.net[2].bias.copy_(torch.arange(6.0) * 0.1)
    path = tmp_path / "decoder_exp3_epoch1.pt"
    torch.save({"epoch": 1, "model_state_dict": model.state_dict()}, path)
    guide = surface.load_guide(str(path), 8)
    maps = guide(torch.zeros(1, 8, 2, 2))
    assert abs(float(maps["opacity_mult"][0, 0, 0].detach()) - (1.0 + np.tanh(0.5) * 0.3)) < 1e-6
    with pytest.raises(RuntimeError):                                     # strict: another architecture's keys do not load
        torch.save({"model_state_dict": {"net.0.weight": torch.zeros(4, 8), "net.2.weight": torch.zeros(6, 4)}}, path)
        surface.load_guide(str(path), 8)
