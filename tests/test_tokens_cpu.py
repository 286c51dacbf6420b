"""Patch-token rows, the parts that need no GPU: the two C declarations and their binding, the ABI version, the
default token window per tower, and the committed fixtures of tests/golden/make_tokens_golden.py."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, ROOT)

from multimodal_embeddings_amd._lib import ABI_VERSION, EXPORTS, Engine  # noqa: E402
from multimodal_embeddings_amd.weights import DINOV2_B14, VIT_B16, VIT_B32  # noqa: E402

DECLARATIONS = [
    "int mme_vit_tokens(mme_ctx* ctx, const uint16_t* patches_dev, int n, int pool_token, int tok0, int ntok, uint16_t* tokens_bf16_dev, "
    "float* emb_f32_dev, uint16_t* emb_bf16_dev, void* stream);",
    "int mme_embed_tokens(mme_ctx* ctx, const uint8_t* pix_dev, const int64_t* offs_host, const int32_t* hw_host, int n, int pool_token, "
    "int tok0, int ntok, uint16_t* tokens_bf16_dev, float* emb_f32_dev, uint16_t* emb_bf16_dev, void* stream);",
]


def test_the_declarations_and_their_binding():
    header = open(os.path.join(ROOT, "include", "mme.h")).read()
    flat = re.sub(r"\s+", " ", header)
    for decl in DECLARATIONS:
        assert decl in flat, decl
        name = decl.split("(")[0].split()[-1]
        assert name in EXPORTS
        assert len(EXPORTS[name][1]) == decl.count(",") + 1, f"{name}: the binding's argument count"
    assert "#define MME_ABI_VERSION 2\n" in header and ABI_VERSION == 2, "exports are added, none changes"


class _Windows(Engine):
    """Engine._token_window on a stated geometry and encoder kind, without a context"""

    def __init__(self, geom, kind):
        self._geom, self._kind = geom, kind

    def __del__(self):
        pass

    def vit_geometry(self):
        return self._geom

    def encoder_info(self):
        return {"kind": self._kind}


@pytest.mark.parametrize("geom, kind, want", [(VIT_B16, "vit", (1, 196)), (VIT_B32, "vit", (1, 49)), (VIT_B16, "clip", (1, 196)),
                                              (DINOV2_B14, "dinov2", (1, 256)), (VIT_B16, "siglip", (0, 196))])
def test_the_default_window_is_the_patch_tokens(geom, kind, want):
    e = _Windows(geom, kind)
    assert e._token_window(None, None)[:2] == want
    first = want[0]
    assert e._token_window(0, None)[:2] == (0, want[1] + first), "ntok defaults to the rest"
    assert e._token_window(5, 3)[:2] == (5, 3)


def test_the_committed_fixtures_are_what_the_maker_describes():
    import make_tokens_golden as mkt

    for tower, (_, geom, _) in mkt.CASES.items():
        path = mkt.out_path(tower)
        assert os.path.getsize(path) < 512 * 1024, "a few hundred KB a file"
        tok = np.load(path)["tokens"]
        tokens = geom.num_patches + (0 if tower == "siglip" else 1)
        assert tok.dtype == np.float16 and tok.shape == (mkt.N_CROPS, tokens, geom.hidden_size) and np.isfinite(tok).all()
        # rows behind a LayerNorm: spread of order one, no two neighbouring rows alike
        assert 0.2 < float(tok.astype(np.float64).std()) < 5.0 and float(np.abs(tok[:, 1:].astype(np.float64) - tok[:, :-1]).max(axis=2).min()) > 0.01


def test_get_patch_embeddings_refuses_the_tile_tower():
    from multimodal_embeddings_amd.embedder import RegionEmbedder

    emb = object.__new__(RegionEmbedder)  # no context: the refusal comes before anything is touched
    emb.encoder = "mllama_tiles"
    with pytest.raises(NotImplementedError, match="encoder 'mllama_tiles'; supported: the single-tile image towers"):
        emb.get_patch_embeddings([np.zeros((8, 8, 3), dtype=np.uint8)])
