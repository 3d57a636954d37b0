"""CPU tests of the recurrent latent layer (rave/blocks.py:295-319 `GRU`): the module keeps the reference's state_dict
layout and initial values, build_v2's `gru_layers` switch leaves every existing model alone, and the C entry points refuse
what they do not build before anything touches a GPU."""
import ctypes as C
import os

import pytest
import torch

RH_ERR_INVALID, RH_ERR_UNSUPPORTED, RH_ERR_WORKSPACE = -1, -2, -3


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return torch.load(os.path.join(golden_dir, "gru_tiny.pt"), weights_only=False)


def test_module_has_the_reference_state_dict_layout(fixture):
    from rave_amd import blocks
    m = blocks.GRU(128, 2)
    got = sorted((k, tuple(v.shape)) for k, v in m.state_dict().items())
    assert got == [(k, tuple(s)) for k, s in fixture["keys_128_2"]]
    assert [k for k, _ in got if not k.startswith("gru.")] == ["gru_state"]
    assert m.enabled is True
    m.disable()
    assert m.enabled is False
    m.enable()
    assert m.enabled is True


@pytest.mark.parametrize("hidden,layers", [(128, 2), (48, 3), (16, 1)])
def test_initial_values_equal_torch_gru_under_the_same_seed(hidden, layers):
    from rave_amd import blocks
    torch.manual_seed(11)
    ref = torch.nn.GRU(input_size=hidden, hidden_size=hidden, num_layers=layers, batch_first=True)
    after_ref = torch.rand(3)
    torch.manual_seed(11)
    m = blocks.GRU(hidden, layers)
    after = torch.rand(3)
    assert [n for n, _ in m.gru.named_parameters()] == [n for n, _ in ref.named_parameters()]
    for (n, p), (_, q) in zip(m.gru.named_parameters(), ref.named_parameters()):
        assert torch.equal(p, q), n
    assert torch.equal(after, after_ref)                 # ... and the generator is left where torch.nn.GRU leaves it


def test_fixture_checkpoint_loads_both_ways(fixture):
    from rave_amd import blocks
    b, h, t, n_layers = fixture["shape"]
    m = blocks.GRU(h, n_layers)
    m.load_state_dict(fixture["state_dict"], strict=True)
    ref = torch.nn.GRU(input_size=h, hidden_size=h, num_layers=n_layers, batch_first=True)
    ref.load_state_dict({k[len("gru."):]: v for k, v in m.state_dict().items() if k.startswith("gru.")}, strict=True)


def test_unbuilt_sizes_are_refused_by_the_module():
    from rave_amd import blocks
    for hidden, layers in ((256, 2), (24, 1), (128, 5), (128, 0)):
        with pytest.raises(NotImplementedError):
            blocks.GRU(hidden, layers)


def test_build_v2_default_is_unchanged_and_gru_layers_shifts_the_decoder():
    from rave_amd import model as M
    kw = dict(capacity=16, latent_size=16, disc_capacity=16)
    torch.manual_seed(0)
    base = M.build_v2(**kw)
    torch.manual_seed(0)
    zero = M.build_v2(gru_layers=0, **kw)
    assert list(base.state_dict()) == list(zero.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(base.state_dict().values(), zero.state_dict().values()))
    assert not any(".gru" in k for k in base.state_dict())
    rec = M.build_v2(gru_layers=2, **kw)
    keys = list(rec.state_dict())
    gru_keys = [k for k in keys if k.startswith("decoder.net.0.")]
    assert sorted(gru_keys) == sorted(
        [f"decoder.net.0.gru.{n}_l{k}" for k in range(2) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        + ["decoder.net.0.gru_state"])

    def shifted(k):
        parts = k.split(".")
        if parts[:2] == ["decoder", "net"]:
            parts[2] = str(int(parts[2]) + 1)
        return ".".join(parts)
    assert [k for k in keys if k not in gru_keys] == [shifted(k) for k in base.state_dict()]
    for k, v in base.state_dict().items():
        assert rec.state_dict()[shifted(k)].shape == v.shape, k


def test_gin_overlay_binds_the_layer_like_hybrid_gin():
    """rave_amd/configs/mi355x_gru.gin carries the generator-side bindings of configs/hybrid.gin:33-38 for the drop-in
    classes (GeneratorV2 calls ``recurrent_layer(latent_size)`` positionally, which gin lets win over the binding -- the
    reference's own file binds latent_size the same way), and the drop-in generator builds with such a callable."""
    import re
    from functools import partial
    from rave_amd import blocks
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "rave_amd", "configs", "mi355x_gru.gin")).read()
    code = "\n".join(ln for ln in text.splitlines() if not ln.lstrip().startswith("#"))
    assert re.search(r"rave_amd\.blocks\.GeneratorV2:\s*\n\s+recurrent_layer = @rave_amd\.blocks\.GRU\s*(\n|$)", code)
    assert re.search(r"rave_amd\.blocks\.GRU:\s*\n\s+latent_size = %LATENT_SIZE\s*\n\s+num_layers = 2\s*\n", code)
    assert "mel" in text.lower() and "not provided" in text.lower()      # the header says what the overlay leaves out
    g = blocks.GeneratorV2(capacity=8, ratios=[4, 2], latent_size=16, kernel_size=3, dilations=[1, 3], data_size=16,
                           recurrent_layer=partial(blocks.GRU, num_layers=2))
    assert isinstance(g.net[0], blocks.GRU) and g.net[0].num_layers == 2
    assert g.net[0].gru.weight_ih_l1.shape == (48, 16)


def test_entry_points_refuse_unbuilt_sizes_and_null_pointers():
    from rave_amd import _lib as L
    lib = L.lib
    for hidden, layers, want in ((16, 1, 1), (128, 4, 1), (48, 2, 1), (24, 1, 0), (256, 2, 0), (0, 1, 0), (144, 1, 0),
                                 (128, 0, 0), (128, 5, 0), (-16, 1, 0)):
        assert lib.rh_gru_supported(hidden, layers) == want, (hidden, layers)
    n = C.c_int64(-7)
    assert lib.rh_gru_workspace_bytes(3, 48, 7, 2, 1, C.byref(n)) == 0 and n.value > 0
    train_bytes = n.value
    assert lib.rh_gru_workspace_bytes(3, 48, 7, 2, 0, C.byref(n)) == 0 and 0 < n.value < train_bytes
    assert lib.rh_gru_workspace_bytes(3, 48, 7, 2, 1, None) == RH_ERR_INVALID

    items = (L.GruItem * 4)()
    for it in items:                                     # never dereferenced: every call below is refused before a launch
        for name, _ in L.GruItem._fields_:
            setattr(it, name, 64)
    p = 64

    def fwd(hidden=48, layers=2, batch=3, t=7, x=p, y=p, ws=p, nbytes=train_bytes, table=items):
        return lib.rh_gru_fwd_f32(x, table, layers, batch, hidden, t, 1, y, ws, nbytes, None)

    def bwd(hidden=48, layers=2, batch=3, t=7, dy=p, x=p, dx=p, ws=p, nbytes=train_bytes, table=items):
        return lib.rh_gru_bwd_f32(dy, x, table, layers, batch, hidden, t, dx, ws, nbytes, None)

    for call in (fwd, bwd):
        for bad in (dict(hidden=24), dict(hidden=256), dict(hidden=0), dict(layers=0), dict(layers=5), dict(t=0),
                    dict(batch=0)):
            assert call(**bad) == RH_ERR_UNSUPPORTED, (call.__name__, bad)
            assert lib.rh_last_error()
            k = next(iter(bad))
            assert lib.rh_gru_workspace_bytes(bad.get("batch", 3), bad.get("hidden", 48), bad.get("t", 7),
                                              bad.get("layers", 2), 1, C.byref(n)) == RH_ERR_UNSUPPORTED, k
        assert b"256" in (call(hidden=256), lib.rh_last_error())[1]
        assert call(x=None) == RH_ERR_INVALID
        assert call(ws=None) == RH_ERR_INVALID
        assert call(table=None) == RH_ERR_INVALID
        assert call(nbytes=train_bytes - 4) == RH_ERR_WORKSPACE
    assert fwd(y=None) == RH_ERR_INVALID
    assert bwd(dy=None) == RH_ERR_INVALID and bwd(dx=None) == RH_ERR_INVALID
    holed = (L.GruItem * 2)()
    for it in holed:
        for name, _ in L.GruItem._fields_:
            setattr(it, name, 64)
    holed[1].w_hh = None
    assert fwd(table=holed) == RH_ERR_INVALID and b"layer 1" in lib.rh_last_error()
    holed[1].w_hh = 64
    holed[0].db_ih = None
    assert bwd(table=holed) == RH_ERR_INVALID and b"layer 0" in lib.rh_last_error()
    # the forward ignores the gradient pointers -- it gets past the table check and is stopped by the short workspace
    assert fwd(table=holed, nbytes=0) == RH_ERR_WORKSPACE
