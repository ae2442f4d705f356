"""Host side of the feature fold (hip.FoldedColor): what is handed to mp_fold_features, how its output is packed, and when.

No device here, so the two native entry points the host calls are stood in for: mp_fold_features by its contract as the header
states it, in fp32 torch, and mp_pack_layers by a recorder.  What is checked against a float64 restatement is then the host's own
work: which layers and columns it pairs, the K-slot order and the 1/K scale of the folded columns, the bias, the hoisted columns,
and the cache key over BOTH modules.  The kernels themselves run in tests/test_feature_fold_gpu.py."""
import numpy as np
import pytest
import torch

from tests import weight_regimes as W


class FakeLib:
    def __init__(self):
        self.folds, self.packs = 0, 0

    def mp_fold_features(self, vc, gc, bc, out_c, in_c, col0, n_feat, v8, g8, b8, in8, out_w, out_b, stream):
        self.folds += 1
        assert tuple(vc.shape) == (out_c, in_c) and tuple(v8.shape) == (1 + n_feat, in8) and in8 <= n_feat
        assert tuple(out_w.shape) == (out_c, in_c) and tuple(out_b.shape) == (out_c,)
        wc = vc if gc is None else vc * (gc.reshape(-1, 1) / vc.norm(dim=1, keepdim=True))
        w8 = v8 if g8 is None else v8 * (g8.reshape(-1, 1) / v8.norm(dim=1, keepdim=True))
        out_w.copy_(wc)
        out_w[:, col0:col0 + n_feat] = 0.0
        out_w[:, col0:col0 + in8] = wc[:, col0:col0 + n_feat] @ w8[1:]
        out_b.copy_(bc + wc[:, col0:col0 + n_feat] @ b8[1:])

    def mp_pack_layers(self, tab, n_layers, ks_in, stream):
        self.packs += 1


@pytest.fixture
def fake(monkeypatch):
    from multiply_amd import hip
    lib = FakeLib()
    monkeypatch.setattr(hip, "lib", lambda: lib)
    monkeypatch.setattr(hip, "stream", lambda: None)
    lib.weights = []          # the `weights` flag of every table the pack is launched with: True = the weights are packed again
    table = hip.PackedNet._table

    def recording(self, weights, hoisted):
        lib.weights.append(bool(weights))
        return table(self, weights, hoisted)
    monkeypatch.setattr(hip.PackedNet, "_table", recording)
    return lib


def pairs(m):
    """(rendering net, its SDF net, ks_in, hoisted vector) of the foreground and the background pair"""
    return [(m.foreground_rendering_network_list[0], m.foreground_implicit_network_list[0], 2, torch.randn(8)),
            (m.bg_rendering_network, m.bg_implicit_network, 3, torch.randn(32))]


@pytest.mark.parametrize("name", W.REGIMES)
def test_folded_plan_against_float64(name, fake):
    from multiply_amd import hip
    from multiply_amd.networks import effective_weight
    m, _, _ = W.regime_networks(name)
    for ren, imp, ks_in, hv in pairs(m):
        fc = hip.FoldedColor(ren, imp, ks_in)
        pk = fc.refresh(hv)
        lin_c, lin_8 = list(ren.layers())[0], list(imp.layers())[-1]
        wc, w8 = effective_weight(lin_c).detach().double(), effective_weight(lin_8).detach().double()
        c0 = hip.feature_col0(ren)
        assert wc.shape[1] == c0 + 256 and w8.shape == (257, 256)
        prod = wc[:, c0:] @ w8[1:]                                        # (out_c, 256): multiplies h7
        want_b = lin_c.bias.detach().double() + wc[:, c0:] @ lin_8.bias.detach().double()[1:]
        # the K-slot matrix the pack kernel builds from the plan: M[r][s] = W[rowmap[r]][colmap[s]] * colscale[s]
        p = pk.plans[0]
        assert p.lin is fc.folded and p.act == hip.ACT_RELU and p.bias_scale == 1.0
        cm, cs = torch.from_numpy(p.colmap(ks_in)).long(), pk.colscales[0].double()
        rows = torch.from_numpy(p.rowmap).long()
        assert rows.tolist() == list(range(wc.shape[0]))
        M = torch.where(cm[None, :] >= 0, fc.folded.weight.double()[rows][:, cm.clamp(min=0)], torch.zeros((), dtype=torch.float64)) * cs
        want = torch.zeros_like(M)
        feat_of_slot = torch.tensor([hip.reg_slot_feature(s) for s in range(256)])
        want[:, :256] = prod[:, feat_of_slot] / hip.SOFTPLUS_K             # h7 arrives as K h7, in the hidden layers' K-slot order
        n_in = c0 - p.hoist[1]
        assert p.hoist == (n_in, c0 - n_in)
        want[:, 256:256 + n_in] = wc[:, :n_in]                             # the input-fed columns, unscaled
        scale = float(want.abs().max())
        assert float((M - want).abs().max()) <= 1e-5 * scale               # fp32 products of 256 terms against float64
        assert float((fc.folded.bias.double() - want_b).abs().max()) <= 1e-5 * max(float(want_b.abs().max()), 1e-30)
        # the hoisted columns are read from the folded weight at every call: they must be the effective weight's
        h0, hn = p.hoist
        assert float((fc.folded.weight[:, h0:h0 + hn].double() - wc[:, h0:h0 + hn]).abs().max()) <= 1e-6 * float(wc.abs().max())
        # every other layer of the rendering network is packed as it is
        plain = hip.rendering_plans(ren)
        assert [q.lin for q in pk.plans[1:]] == [q.lin for q in plain[1:]]
        for q, r in zip(pk.plans[1:], plain[1:]):
            assert (q.act, q.out_chunk, q.scale, q.in_scale) == (r.act, r.out_chunk, r.scale, r.in_scale)
            assert np.array_equal(q.colmap(ks_in), r.colmap(ks_in)) and np.array_equal(q.rowmap, r.rowmap)
        # the SDF side: the 'sdf' plan ends in the sdf row alone, one chunk returned in fp32 -- 8 chunks fewer than 'full'
        sdf = hip.PackedNet(hip.implicit_plans(imp, "sdf"), ks_in, "cpu")
        full = hip.PackedNet(hip.implicit_plans(imp, "full"), ks_in, "cpu")
        last = sdf.net.layer[sdf.net.n_layers - 1]
        assert (last.n_chunk, last.out_chunk, last.act, last.use_reg) == (1, 0, hip.ACT_NONE, 1)
        assert sdf.plans[-1].rowmap.tolist() == [0] + [-1] * 31
        assert full.net.total_chunks == sdf.net.total_chunks + 8


def test_repacks_when_a_parameter_of_either_module_changed(fake):
    from multiply_amd import hip
    m, _, _ = W.regime_networks("geometric")
    for ren, imp, ks_in, hv in pairs(m):
        fake.folds, fake.weights[:] = 0, []
        fc = hip.folded_color(ren, imp, ks_in)
        assert hip.folded_color(ren, imp, ks_in) is fc
        lin_c, lin_8 = list(ren.layers())[0], list(imp.layers())[-1]

        def call():
            n = len(fake.weights)
            fc.refresh(hv)
            assert len(fake.weights) == n + 1                 # one pack launch per call: the hoisted bias at the least
            return fake.folds, fake.weights[-1]
        assert call() == (1, True)                            # first use: fold + full pack
        assert call() == (1, False)                           # nothing changed: the hoisted bias only
        assert call() == (1, False)
        with torch.no_grad():
            (lin_c.weight_v if hasattr(lin_c, "weight_v") else lin_c.weight).mul_(1.5)
        assert call() == (2, True)                            # the rendering network's first layer
        assert call() == (2, False)
        with torch.no_grad():
            lin_8.bias.add_(0.25)
        assert call() == (3, True)                            # the SDF network's last layer
        with torch.no_grad():
            (lin_8.weight_v if hasattr(lin_8, "weight_v") else lin_8.weight).mul_(0.5)
        assert call() == (4, True)
        assert call() == (4, False)
        with torch.no_grad():
            list(ren.layers())[1].bias.add_(1.0)
        assert call() == (4, True)                            # a later rendering layer: packed again, no new product
        hip.invalidate_packed()                               # a parameter update that bumps no version counter
        assert call() == (5, True)
        assert call() == (5, False)
        # the values follow the change: the folded bias holds the new product
        from multiply_amd.networks import effective_weight
        wc = effective_weight(lin_c).detach().double()
        want_b = lin_c.bias.detach().double() + wc[:, fc.col0:] @ lin_8.bias.detach().double()[1:]
        assert float((fc.folded.bias.double() - want_b).abs().max()) <= 1e-5 * float(want_b.abs().max())
