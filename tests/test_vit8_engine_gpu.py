"""VSMConfig.vit_w8a8 through the engine (MI355X): the block linears of the CLIP and OWL-ViT towers on the fp8 MFMA for tower calls of
>= 1024 rows, against tests/_vit8_oracle.py (the fake-quant restatement of oracle.vit_tower) and against the bf16 engine.

Two configs with a tiny LLM: narrow towers (256 wide) and the real tower widths (CLIP 1024 / 4096, OWL-ViT 768 / 3072), two blocks each.
Four crops at 224 px give 1028 CLIP rows (the smallest call that takes the fp8 path, with a ragged last row tile) and 9220 OWL rows.

Gates (taps clip_features and owl_feats):
  * engine8 vs engine16 in (1e-4, 0.15): the quantisation really ran and costs a few percent (the oracle pair alone: 4.1e-2);
  * engine8 vs the fake-quant oracle <= 6 x max(noise16, 5e-3), noise16 = the bf16 engine's distance to the fp32 vit_tower on the same
    tap — factor and floor of tests/test_engine_gpu.py::test_w8a8_mode_matches_fake_quant_oracle.  With noise16 ~ 5e-3 the gate is
    ~ 3e-2, below the 4.1e-2 an engine that ignored the quantisation would score.
Measured on the MI355X (this file, -s): see DESIGN.md §9."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _vit8_oracle
from oracle import vsm_oracle
from vstar_amd import _lib
from vstar_amd.config import VSMConfig
from vstar_amd.engine import VstarEngine, loc_positions
from vstar_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

WIDTHS = {"narrow": dict(clip_hidden=256, clip_heads=4, clip_mlp=1024, owl_hidden=256, owl_heads=4, owl_mlp=512),
          "real": dict(clip_hidden=1024, clip_heads=16, clip_mlp=4096, owl_hidden=768, owl_heads=12, owl_mlp=3072)}
B, L = 4, 24


def rel_l2(got, ref):
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30))


class _Model:
    """One config: weights, inputs, engines by (vit_w8a8, llm_w8a8) and the CPU references, each made once."""

    def __init__(self, name):
        self.kw = WIDTHS[name]
        self.cfg = VSMConfig.tiny(**self.kw)
        self.sd = random_state_dict(self.cfg, seed=0, dtype=torch.bfloat16)
        g = torch.Generator().manual_seed(78)
        self.clip = torch.randn(B, 3, 224, 224, generator=g).bfloat16()
        self.owl = torch.randn(B, 3, 768, 768, generator=g).bfloat16()
        loc_id = self.cfg.llm_vocab - 1
        ids = torch.randint(3, loc_id - 3, (B, L), generator=g)
        ids[:, 0] = 1
        ids[:, 5] = -200
        ids[:, L - 3] = loc_id
        self.ids = ids.numpy()
        self.loc = loc_positions(self.ids, loc_id, self.cfg.n_img_tokens)
        self.engines, self.refs = {}, None

    def engine(self, vit, llm=0):
        if (vit, llm) not in self.engines:
            eng = VstarEngine(VSMConfig.tiny(vit_w8a8=vit, llm_w8a8=llm, **self.kw), 0)
            eng.load_state_dict(self.sd)
            self.engines[(vit, llm)] = eng
        return self.engines[(vit, llm)]

    def score(self, eng, n=B):
        out = eng.score_batch(self.clip[:n], self.owl[:n], self.ids[:n], self.loc[:n])
        c = self.cfg
        taps = {"clip_features": eng.debug_read("clip_features", n * (c.n_img_tokens + 1) * c.clip_hidden).reshape(n, c.n_img_tokens + 1, -1)[:, 1:],
                "owl_feats": eng.debug_read("owl_feats", n * 2304 * c.owl_hidden).reshape(n, 2304, -1)}
        return out, taps

    def references(self):
        """fp32 vit_tower (the yardstick of the bf16 engine's noise) and the fake-quant towers in the engine's storage type."""
        if self.refs is None:
            c, sd32 = self.cfg, {k: v.float() for k, v in self.sd.items()}
            self.refs = {
                "plain": {"clip_features": vsm_oracle.clip_features(sd32, self.clip.float(), c.clip_heads, c.clip_layers, c.clip_select_layer).numpy(),
                          "owl_feats": vsm_oracle.owl_visual_embs(sd32, self.owl.float(), c.owl_heads, c.owl_layers).reshape(B, 2304, -1).numpy()},
                "quant": {"clip_features": _vit8_oracle.clip_features8(self.sd, c, self.clip).float().numpy(),
                          "owl_feats": _vit8_oracle.owl_feats8(self.sd, c, self.owl).float().reshape(B, 2304, -1).numpy()}}
        return self.refs

    def close(self):
        for e in self.engines.values():
            e.close()
        self.engines.clear()


@pytest.fixture(scope="module", params=["narrow", "real"])
def model(request, cuda):
    m = _Model(request.param)
    yield m
    m.close()


def test_towers_match_the_fake_quant_oracle(model):
    e8, e16 = model.engine(1), model.engine(0)
    _, t8 = model.score(e8)
    assert e8.w8a8_vit_active() == 3
    _, t16 = model.score(e16)
    assert e16.w8a8_vit_active() == 0
    refs = model.references()
    for tap in ("clip_features", "owl_feats"):
        d_engines = rel_l2(t8[tap], t16[tap])
        noise16 = rel_l2(t16[tap], refs["plain"][tap])
        d_oracle = rel_l2(t8[tap], refs["quant"][tap])
        d_pair = rel_l2(refs["quant"][tap], refs["plain"][tap])
        gate = 6 * max(noise16, 5e-3)
        print(f"VIT8 {tap}: engine8 vs engine16 {d_engines:.3e}; engine8 vs fake-quant oracle {d_oracle:.3e} (gate {gate:.3e}, "
              f"share {d_oracle / gate:.2f}); noise16 {noise16:.3e}; fake-quant oracle vs fp32 tower {d_pair:.3e}")
        assert 1e-4 < d_engines < 0.15, (tap, d_engines)
        assert d_oracle <= gate, (tap, d_oracle, gate)


def test_small_calls_run_the_bf16_path_bit_for_bit(model):
    """One crop: 257 CLIP rows stay on the bf16 path of the engine without the mode (same bits); the OWL-ViT tower has 2305 rows."""
    e8, e16 = model.engine(1), model.engine(0)
    _, t8 = model.score(e8, 1)
    mask = e8.w8a8_vit_active()
    _, t16 = model.score(e16, 1)
    assert np.array_equal(t8["clip_features"], t16["clip_features"])
    assert mask & 1 == 0 and mask & 2 == 2
    assert e16.w8a8_vit_active() == 0


def test_with_the_llama_linears_on_fp8_too(model):
    """vit_w8a8 is independent of llm_w8a8: both on gives finite outputs, and the tower launches are counted as fp8 launches."""
    counts = {}
    for vit in (0, 1):
        eng = model.engine(vit, 1)
        eng.profile(True)
        out, _ = model.score(eng)
        counts[vit] = eng.profile_read_fp8()[1]
        eng.profile(False)
        assert eng.w8a8_vit_active() == (3 if vit else 0)
        assert np.isfinite(out["pred_logits"]).all() and np.isfinite(out["low_res_masks"]).all()
    c = model.cfg
    # four fp8 linears per executed block of each tower, on top of the LLaMA launches both engines make
    assert counts[1] - counts[0] == 4 * (c.clip_blocks + c.owl_layers), counts


def test_vit_w8a8_other_values_fail_at_create(cuda):
    with pytest.raises(_lib.VstarError, match="vit_w8a8"):
        VstarEngine(VSMConfig.tiny(vit_w8a8=2), 0)


def test_env_target_llm_w8a8_engine(cuda):
    """An engine created with llm_w8a8 = 1 and vit_w8a8 = 0: the towers run fp8 exactly when VSTAR_W8A8_VIT=1 was in the environment at
    vstar_create (the subprocess test below sets it; in the suite's own process it is unset and the config decides)."""
    m = _Model("narrow")
    try:
        eng = m.engine(0, 1)
        m.score(eng)
        assert eng.w8a8_vit_active() == (3 if os.environ.get("VSTAR_W8A8_VIT") == "1" else 0)
    finally:
        m.close()


def test_env_switch_turns_the_towers_on_for_llm_w8a8_engines(cuda):
    env = dict(os.environ, VSTAR_W8A8_VIT="1")
    r = subprocess.run([sys.executable, "-m", "pytest", __file__, "-q", "-m", "gpu", "-k", "test_env_target_llm_w8a8_engine", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-2000:] + r.stderr[-1000:]
