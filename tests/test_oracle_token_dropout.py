"""oracle/token_dropout.py (the host restatement of the token encoder's dropout masks, csrc/token_encoder.h tok_hash /
make_drop) and the masked ``oracle.student.encoder_layer`` the train-mode GPU tests use as their float64 reference."""
import numpy as np
import torch
import torch.nn as nn

# (seed, site, element, tok_hash)
PINNED = [
    (0, 0, 0, 0), (0, 0, 1, 1469096322), (0, 1, 0, 4048596679), (0, 3, 70001, 3639788076), (0, 7, 393215, 1832313650),
    (0, 6, 4294967295, 849903007),
    (12345, 0, 31, 1090369818), (12345, 1, 70001, 1651962559), (12345, 3, 0, 2885538855), (12345, 6, 393215, 3642234420),
    (12345, 7, 1, 1335389999),
    (0x123456789ABCDEF, 0, 0, 2368264961), (0x123456789ABCDEF, 1, 70001, 2740052366),
    (0x123456789ABCDEF, 3, 393215, 442405835), (0x123456789ABCDEF, 6, 31, 3164607886),
    (0x123456789ABCDEF, 7, 4294967295, 156397833),
    (0x3FFFFFFF00000001, 0, 1, 2102258842), (0x3FFFFFFF00000001, 1, 393215, 2049888846),
    (0x3FFFFFFF00000001, 3, 70001, 3212382052), (0x3FFFFFFF00000001, 6, 0, 3350611386),
    (0x3FFFFFFF00000001, 7, 31, 2783737345),
]


def test_tok_hash_reproduces_the_header():
    """The literal values are ``hash`` lines of tools/draws_check.cpp, a host program that includes csrc/tok_hash.h itself
    (``g++ -std=c++17 tools/draws_check.cpp -o draws_check && ./draws_check`` regenerates them; tests/test_draws_cpu.py
    compares the list with its output).  Seeds with a zero and a non-zero high word (the ``seed >> 32`` add), sites of both
    layers, elements above 2^16 and the last uint32."""
    from oracle import token_dropout as td
    for seed, site, idx, want in PINNED:
        assert int(td.tok_hash(seed, site, np.array([idx]))[0]) == want, (seed, site, idx)
    # vectorised over an index array = element by element; indices are taken modulo 2^32
    seed = 0x3FFFFFFF00000001
    idx = np.array([r[2] for r in PINNED if r[0] == seed and r[1] == 3], dtype=np.uint64)
    want = [r[3] for r in PINNED if r[0] == seed and r[1] == 3]
    assert td.tok_hash(seed, 3, idx).tolist() == want
    assert td.tok_hash(seed, 3, idx + np.uint64(2 ** 32)).tolist() == want
    assert td.tok_hash(seed, 3, idx).dtype == np.uint32


def test_threshold_scale_and_keep_rate():
    from oracle import token_dropout as td
    assert int(td.threshold(0.1)) == 429496736            # float32(0.1) * 2^32, not 0.1 * 2^32 = 429496729
    assert int(td.threshold(0.5)) == 2147483648
    assert int(td.threshold(0.3)) == 1288490240
    assert int(td.threshold(0.0)) == 0
    idx = np.arange(393216)
    m = td.keep_scale(0.1, 0x2B5C9D1E00F0A7C3, 5, idx)
    assert set(np.unique(m).tolist()) == {0.0, 1.0 / (1.0 - float(np.float32(0.1)))}
    assert abs((m != 0).mean() - 0.9) < 2e-3              # 3 sigma of 393216 Bernoulli(0.9) draws = 1.4e-3
    assert np.array_equal(m != 0, td.tok_hash(0x2B5C9D1E00F0A7C3, 5, idx) >= 429496736)
    assert np.array_equal(td.keep_scale(0.5, 7, 0, idx[:64]) != 0, td.tok_hash(7, 0, idx[:64]) >= 2 ** 31)
    assert set(np.unique(td.keep_scale(0.5, 7, 0, idx[:64])).tolist()) == {0.0, 2.0}


def test_p_zero_masks_nothing():
    from oracle import token_dropout as td
    assert np.array_equal(td.keep_scale(0.0, 99, 3, np.arange(1000)), np.ones(1000))
    for m in td.layer_masks(3, 2, 2, 128, 0.0, 99, 1):
        assert np.array_equal(m, np.ones_like(m))


def test_layer_masks_shapes_sites_and_element_numbers():
    from oracle import token_dropout as td
    B, S, H, ff, p, seed = 5, 3, 2, 128, 0.3, 0x123456789ABCDEF
    for l in (0, 1):
        att, sa, act, out = td.layer_masks(B, S, H, ff, p, seed, l)
        assert att.shape == (B, H, S, S) and sa.shape == (B, S, 32) and act.shape == (B, S, ff) and out.shape == (B, S, 32)
        b, h, i, j, s, f, c = 3, 1, 2, 1, 2, 17, 101
        assert att[b, h, i, j] == td.keep_scale(p, seed, 4 * l + 0, np.array(((b * H + h) * S + i) * S + j))
        assert sa[b, s, f] == td.keep_scale(p, seed, 4 * l + 1, np.array((b * S + s) * 32 + f))
        assert act[b, s, c] == td.keep_scale(p, seed, 4 * l + 2, np.array((b * S + s) * ff + c))
        assert out[b, s, f] == td.keep_scale(p, seed, 4 * l + 3, np.array((b * S + s) * 32 + f))
        assert not np.array_equal(att[:, 0], att[:, 1])        # the two heads carry different masks
        assert not np.array_equal(sa, out)                     # as do the two branch sites
    assert not np.array_equal(td.layer_masks(B, S, H, ff, p, seed, 0)[3], td.layer_masks(B, S, H, ff, p, seed, 1)[3])


def _layer_sd(dtype=torch.float64):
    torch.manual_seed(0)
    layer = nn.TransformerEncoderLayer(d_model=32, nhead=2, dim_feedforward=128, activation="gelu", batch_first=True,
                                       norm_first=True)
    return {k: (v + 0.1 * torch.randn_like(v)).to(dtype) for k, v in layer.state_dict().items()}


def test_masked_encoder_layer_with_all_ones_is_the_unmasked_layer():
    from oracle import student as os_
    sd = _layer_sd()
    x = torch.randn(4, 3, 32, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    ones = (torch.ones(4, 2, 3, 3, dtype=torch.float64), torch.ones(4, 3, 32, dtype=torch.float64),
            torch.ones(4, 3, 128, dtype=torch.float64), torch.ones(4, 3, 32, dtype=torch.float64))
    assert torch.equal(os_.encoder_layer(x, sd, 2, ones), os_.encoder_layer(x, sd, 2))
    assert torch.equal(os_.encoder_layer(x, sd, 2, None), os_.encoder_layer(x, sd, 2))


def test_masked_encoder_layer_places_the_masks_like_torch():
    """Mask placement against nn.TransformerEncoderLayer itself: a zero mask at one site removes exactly what torch's
    module loses when that site's dropout is p = 1 in train mode (F.dropout with p = 1 returns zeros)."""
    from oracle import student as os_
    sd = _layer_sd()
    layer = nn.TransformerEncoderLayer(d_model=32, nhead=2, dim_feedforward=128, activation="gelu", batch_first=True,
                                       norm_first=True).double()
    layer.load_state_dict(sd)
    x = torch.randn(4, 3, 32, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    shapes = [(4, 2, 3, 3), (4, 3, 32), (4, 3, 128), (4, 3, 32)]
    for site in range(4):
        for m in (layer.dropout, layer.dropout1, layer.dropout2):
            m.p = 0.0
        layer.self_attn.dropout = 0.0
        if site == 0:
            layer.self_attn.dropout = 1.0
        else:
            (layer.dropout1, layer.dropout, layer.dropout2)[site - 1].p = 1.0
        masks = tuple(torch.zeros(s, dtype=torch.float64) if k == site else torch.ones(s, dtype=torch.float64)
                      for k, s in enumerate(shapes))
        want = layer.train()(x)
        got = os_.encoder_layer(x, sd, 2, masks)
        assert (got - want).abs().max() <= 1e-12, site
        assert (got - os_.encoder_layer(x, sd, 2)).abs().max() > 1e-3, site


def test_masked_encoder_layer_gradcheck():
    """The float64 autograd of the masked layer is the reference for every train-mode gradient: gradcheck it at
    (2, 3, 32) with the masks of a real seed, p = 0.3, w.r.t. the input and every parameter."""
    from oracle import student as os_
    from oracle import token_dropout as td
    sd = _layer_sd()
    names = list(sd)
    masks = td.stack_masks(2, 3, 2, 128, 0.3, 0x3FFFFFFF00000001, 2)[1]
    assert all(float(m.min()) == 0.0 for m in masks)             # every site drops something in this draw
    x = torch.randn(2, 3, 32, dtype=torch.float64, generator=torch.Generator().manual_seed(3)).requires_grad_(True)
    params = [sd[k].clone().requires_grad_(True) for k in names]

    def f(x, *ps):
        return os_.encoder_layer(x, dict(zip(names, ps)), 2, masks)

    assert torch.autograd.gradcheck(f, (x, *params), eps=1e-6, atol=1e-5, rtol=1e-4)


def test_decode_threads_the_masks_to_every_layer():
    from oracle import student as os_
    from oracle import token_dropout as td
    sd = {}
    for l in (0, 1):
        sd.update({f"decoder.sa_decoder.layers.{l}.{k}": v for k, v in _layer_sd().items()})
    g = torch.Generator().manual_seed(4)
    sd["decoder.output_layers.0.weight"] = torch.randn(16, 96, dtype=torch.float64, generator=g) * 0.1
    sd["decoder.output_layers.0.bias"] = torch.zeros(16, dtype=torch.float64)
    sd["latent_predictor.0.weight"] = torch.randn(6, 16, dtype=torch.float64, generator=g)
    sd["latent_predictor.0.bias"] = torch.zeros(6, dtype=torch.float64)
    tok = torch.randn(5, 3, 32, dtype=torch.float64, generator=g)
    masks = td.stack_masks(5, 3, 2, 128, 0.1, 77, 2)
    ones = [tuple(torch.ones_like(m) for m in layer) for layer in masks]
    base = os_.decode(sd, tok)
    assert torch.equal(os_.decode(sd, tok, masks=ones), base)
    assert not torch.equal(os_.decode(sd, tok, masks=[masks[0], ones[1]]), base)
    assert not torch.equal(os_.decode(sd, tok, masks=[ones[0], masks[1]]), base)
