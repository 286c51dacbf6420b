"""Host mirror of deprecated_package/embedder.py over the HIP engine.

Same surface as the reference's `MmE5MllamaEmbedder` (embedder.py:37-254):

    embedder = RegionEmbedder()                       # embedder.py:42
    vecs = embedder.get_image_embeddings(paths)       # embedder.py:141  list[list[float] | None]
    vec  = embedder.embed(region)                     # north_star: embed(region) -> vec

and the same error behaviour: `[]` for an empty list (:154-155), a `None` hole for any
item that fails to load, logged, never raised (:135-137), `[None]` for a failed single
query (:183-185).  What changes is the execution model: the reference loops one image per
forward on one thread per GPU (:104,:208); here the decoded crops of a call are packed
into one device buffer and go through K1 (resize/normalise/patchify) and the batched
bf16 MFMA ViT forward in `mme_embed` calls over bounded groups.  Under a launcher (LOCAL_RANK set)
one process drives one GPU and sharding a corpus across the 8 GPUs of a node is dist.py's job;
constructed plainly, as the reference's callers do, the embedder holds one context per visible
GPU (`gpu_count`, embedder.py:54-65) and fans a call out `i % n_devices` on one thread per
context (embedder.py:191-224).

There is no CPU path: constructing the embedder without libmme.so or without a GPU
raises `MmeError`.
"""
from __future__ import annotations

import logging
from concurrent.futures import ThreadPoolExecutor
import os

import numpy as np

from . import config
from ._lib import Engine, MmeError, ResizeSpec, lanczos_geometry_ok, lanczos_workspace  # noqa: F401
from .staging import ResultRing, Stage, _Null, current_stream, new_event, new_stream, on, packed_layout  # noqa: F401
from .weights import TILE_VIT

logger = logging.getLogger("multimodal_embeddings_amd")


def last_pooling(last_hidden_state, attention_mask, normalize=True):
    """embedder.py:17-34, tensor-for-tensor (torch, any device).

    Kept for API parity; inside the engine the same computation is kernel K8
    (`pool_ln_l2`), which gathers the pooled row straight from the residual stream.
    """
    import torch

    sequence_lengths = attention_mask.sum(dim=1) - 1
    batch_size = last_hidden_state.shape[0]
    reps = last_hidden_state[torch.arange(batch_size, device=last_hidden_state.device), sequence_lengths]
    if normalize:
        reps = torch.nn.functional.normalize(reps, p=2, dim=-1)
    return reps


def convert_to_rgb(image):
    """What the Mllama processor does to a non-RGB image before resizing (transformers
    image_processing_pil_mllama.py:196-211): composite over a WHITE background through RGBA, so transparent
    areas come out white (a plain `.convert("RGB")` would expose the colour stored under the alpha)."""
    from PIL import Image

    if image.mode == "RGB":
        return image
    rgba = image.convert("RGBA")
    background = Image.new("RGBA", rgba.size, (255, 255, 255))
    return Image.alpha_composite(background, rgba).convert("RGB")


def capped_size(h: int, w: int):
    """(new_h, new_w) of the 8000-pixel cap for an image with a side over it: the reference's own expression
    (embedder.py:110-114), evaluated as Python evaluates it there.  It gives 7999 for some long sides and 0 for a short
    side of one pixel (Pillow then raises); neither is "fixed" here."""
    scale = config.MAX_IMAGE_HEIGHT_AND_WIDTH / max(w, h)
    return int(h * scale), int(w * scale)


def _load_rgb(item):
    """path | PIL.Image | uint8[h,w,3] -> contiguous uint8[h,w,3] (embedder.py:107-114)."""
    from PIL import Image

    if isinstance(item, np.ndarray):
        a = item
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"array crops must be uint8[h,w,3], got {a.dtype}{a.shape}")
        h, w = a.shape[:2]
        if h == 0 or w == 0:
            raise ValueError("empty image")
        if max(h, w) <= config.MAX_IMAGE_HEIGHT_AND_WIDTH:
            return np.ascontiguousarray(a)
        image = Image.fromarray(a)
    elif isinstance(item, (str, os.PathLike)):
        image = Image.open(item)
    else:
        image = item  # PIL image
    if image.size[0] > config.MAX_IMAGE_HEIGHT_AND_WIDTH or image.size[1] > config.MAX_IMAGE_HEIGHT_AND_WIDTH:
        scale = config.MAX_IMAGE_HEIGHT_AND_WIDTH / max(image.size)
        image = image.resize((int(image.size[0] * scale), int(image.size[1] * scale)), Image.LANCZOS)
    a = np.asarray(convert_to_rgb(image))
    if a.shape[0] == 0 or a.shape[1] == 0:
        raise ValueError("empty image")
    return np.ascontiguousarray(a)


class _Oversized:
    """An RGB item over the 8000-pixel cap on its way to the device UNCAPPED: `raw` uint8[h, w, 3] as decoded, and the
    size the reference's cap gives it.  The consumer thread shrinks it there (Engine.lanczos_resize) before the pass."""

    def __init__(self, raw, new_h, new_w):
        self.raw, self.new_h, self.new_w = raw, int(new_h), int(new_w)
        self.shape = (self.new_h, self.new_w, 3)  # of the crop the pass sees
        self.work = lanczos_workspace(raw.shape[0], raw.shape[1], self.new_h, self.new_w)
        # what the item takes of a group's packed buffer: the capped image, the raw pixels and the resize's workspace
        self.nbytes = self.new_h * self.new_w * 3 + int(raw.nbytes) + self.work


def _load_for_device(item):
    """`_load_rgb` for the embed pipelines: the same array for every item but one kind -- an RGB item (a uint8[h, w, 3]
    array, a PIL / file image of mode "RGB") with a side over the cap whose geometry mme_lanczos_resize accepts comes back
    as `_Oversized`, uncapped.  Other modes (RGBA resizes premultiplied, P / 1 resize NEAREST), geometry outside the
    entry's range and a cap that leaves a side of zero pixels (Pillow raises) keep the host path, exactly as before."""
    from PIL import Image

    cap = config.MAX_IMAGE_HEIGHT_AND_WIDTH
    if isinstance(item, np.ndarray):
        a = item
        if a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3 and min(a.shape[:2]) > 0 and max(a.shape[:2]) > cap:
            nh, nw = capped_size(a.shape[0], a.shape[1])
            if lanczos_geometry_ok(a.shape[0], a.shape[1], nh, nw):
                return _Oversized(np.ascontiguousarray(a), nh, nw)
        return _load_rgb(item)
    image = Image.open(item) if isinstance(item, (str, os.PathLike)) else item
    w, h = image.size
    if image.mode == "RGB" and max(w, h) > cap:
        nh, nw = capped_size(h, w)
        if lanczos_geometry_ok(h, w, nh, nw):
            raw = np.ascontiguousarray(np.asarray(image))
            if raw.dtype == np.uint8 and raw.shape == (h, w, 3):
                return _Oversized(raw, nh, nw)
    return _load_rgb(image)


def _load_item(pair):
    """(index, item) -> (index, decoded item | None): an item that cannot be read is logged and becomes a hole."""
    i, item = pair
    try:
        return i, _load_for_device(item)  # looked up per call: tools swap the loader at module level
    except Exception as e:  # embedder.py:135-137
        logger.error(f"Error processing image {item if isinstance(item, (str, os.PathLike)) else type(item)}: {e}")
        return i, None


def _decoded_groups(items, step, group_bytes):
    """The front end of both embed paths: [(index, item)] in parts of `step` items, each decoded and cut into groups of at
    most `group_bytes` of pixels.  Yields per part (indices that failed to load, [[(index, decoded item)]])."""
    for g0 in range(0, len(items), step):
        part = items[g0 : g0 + step]
        # PNG decode is the slow part of a call and Pillow releases the GIL while decoding
        if len(part) > 4 and not all(isinstance(it, np.ndarray) for _, it in part):
            with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1, len(part))) as pool:
                loaded = list(pool.map(_load_item, part))
        else:
            loaded = [_load_item(pr) for pr in part]
        groups, group, nbytes = [], [], 0
        for i, a in loaded:
            if a is None:
                continue
            if group and nbytes + a.nbytes > group_bytes:
                groups.append(group)
                group, nbytes = [], 0
            group.append((i, a))
            nbytes += a.nbytes
        if group:
            groups.append(group)
        yield [i for i, a in loaded if a is None], groups


class RegionEmbedder:
    """Drop-in for `MmE5MllamaEmbedder` on one MI355X."""

    GROUP_BYTES = 1 << 30  # packed pixels per mme_embed call (pinned staging + device copy stay bounded)
    TILE_GROUP_CROPS = 32  # crops per pass of the tile-ViT option (15 MB of f32 pixel values and ~230 MB of workspace each)

    def __init__(self, model_name=config.DEFAULT_MODEL_NAME, device=None, gpu_count=None, *, weights=None,
                 seed: int = 1, pool: str = "cls", chunk: int | None = None, engine: Engine | None = None, devices=None,
                 encoder: str = "vit_b16", geometry=None, prune_last_layer: bool | None = None, allow_synthetic: bool = True,
                 resize_rule: str | None = None, text_tower=None, tokenizer=None, lm_geometry=None, prompt_ids=None):
        """`model_name`: a LOCAL checkpoint directory (config.json + model.safetensors | shards | pytorch_model.bin, optionally
        preprocessor_config.json) is read once (checkpoint.read_checkpoint), loaded into every context in the file's own dtype
        and its image_mean / image_std applied; `self.checkpoint` keeps it.  Any other name is never fetched: the encoder runs
        on seeded synthetic weights with one WARNING, or raises with `allow_synthetic=False`.  `weights=` (a dict) wins.
        `encoder`: "vit_b16" (exactly ViT-B/16), "vit" (any ViT/16 or ViT/32 @224 of the supported family -- ViT-S, -B, -L widths,
        weights.SUPPORTED_VIT: a checkpoint directory brings its own geometry in config.json, seeded weights take
        `geometry=`, e.g. weights.VIT_L16 or weights.VIT_B32, a `weights=` dict is sized by its tensors), "clip" (a CLIP ViT/16 or ViT/32 image tower of
        the same family: pre-LN, QuickGELU or GELU, visual projection; a checkpoint directory of CLIPVisionModel[WithProjection]
        or a whole CLIPModel, seeded weights at `geometry=` a weights.CLIPGeometry (weights.CLIP_B32 is clip-vit-base-patch32), default CLIP-B/16, or a `weights=` dict in
        transformers' names, whose activation `geometry=` names when it is not QuickGELU), "siglip_vit" (a SigLIP ViT/16 @224 image
        tower: 196 tokens, tanh-GELU, the attention-pooling head; a checkpoint directory of SiglipVisionModel or a whole
        SiglipModel, seeded weights at `geometry=` a weights.SiglipGeometry, default SigLIP-B/16, or a `weights=` dict in
        transformers' names; `pool` must stay at its default, the head pools), "dinov2" (a DINOv2 ViT/14 @224 image tower:
        257 tokens, LayerScale, `pooler_output`; a checkpoint directory of Dinov2Model -- dinov2-small, -base, -large -- whose
        position table is interpolated to 16 x 16 once at load, seeded weights at `geometry=` a weights.Dinov2Geometry, default
        weights.DINOV2_B14, or a `weights=` dict in transformers' names; it has no text tower) or "mllama_tiles".
        `self.embed_dim` is the width of the vectors this object returns (a CLIP tower's projection_dim).
        `pool`: "cls" or "last" return one token row; "mean" (encoder "vit" and "dinov2") returns the L2-normalised mean of the
        final-LayerNorm patch rows the crop covers on the 224 x 224 canvas -- under the fit-and-pad rule most of a column's or a
        strip's canvas is padding, which stays out of the mean -- and "cls+mean" the class row and that mean side by side under
        one L2 norm (`embed_dim` = 2 x hidden; transformers' Dinov2ForImageClassification feature).  DESIGN.md 4.26.
        `resize_rule`: how K1 makes the 224 x 224 pixels of a crop.  None and "fit_pad" are the aspect-preserving BILINEAR
        fit with zero padding; "clip" is CLIPImageProcessor's shortest-edge-224 BICUBIC resize + centre crop (the single-tile
        encoders only; a checkpoint's preprocessor_config.json must then describe exactly that rule).  It is set on every
        engine of this object; None leaves a caller's `engine=` as it is.  "checkpoint" reads the rule the model was trained
        under from the directory's preprocessor_config.json (checkpoint.resize_spec_of: ViT's and SigLIP's exact 224 x 224
        resize, DINOv2's shortest-edge-256 BICUBIC resize + centre crop, ...; a missing file or a rule K1 does not run is an
        error) and a `ResizeSpec` names such a rule directly; `self.resize_rule` is then "spec" and `self.resize_spec` the spec.
        Neither is ever a default.
        `text_tower`: the text tower behind `get_text_embeddings` (CLIP's; SigLIP's under encoder="siglip_vit"), in the FIRST engine only.  None: nothing is loaded
        now; the first `get_text_embeddings` loads it if `model_name` is a checkpoint directory that holds one.  True: load
        now (from that directory, or seeded CLIP_TEXT_B-shaped weights projecting to this object's `embed_dim` beside a seeded
        image side).  A directory path or a `weights.clip_text_tensor_specs` dict: load that.  False: never.
        Under encoder="siglip_vit" the tower is SigLIP's (64 tokens, `weights.siglip_text_tensor_specs`, a whole SiglipModel or
        a SiglipTextModel directory): True beside seeded or caller's image weights seeds a tower of the image tower's width
        (SIGLIP_TEXT_B at 768); its projection must equal `embed_dim`.  None beside seeded or vision-only weights loads nothing.
        `tokenizer`: a callable str -> list[int] or a transformers tokenizer; by default transformers' CLIPTokenizer is read
        from the tower's directory on first use (local files only).  Token ids need no tokenizer.
        encoder="mllama": the tile tower of "mllama_tiles" AND the Mllama language tower with cross-attention in
        every context: images are embedded through both under the prompt `prompt_ids` (token ids, the image token among them;
        by default `MLLAMA_PROMPT`, the reference's prompt, through `tokenizer=`), texts through the language tower
        alone; `embed_dim` is the text hidden size.  Seeded weights take `geometry=` (a weights.TileViTGeometry) and
        `lm_geometry=` (a weights.MllamaLMGeometry whose vision_output_dim is the tile tower's output width; default
        weights.MLLAMA_LM_11B); a checkpoint directory of MllamaForConditionalGeneration (mmE5's) brings both towers, the
        projector and, where it holds tokenizer files, the tokenizer (local files only).  A str prompt or query needs a
        tokenizer; without one only token ids are taken."""
        import torch

        from .checkpoint import check_resize_rule, read_checkpoint, resolve_model_source
        from .encoders import ENCODER_TABLE

        self.torch = torch
        self.model_name = model_name
        self.checkpoint = None
        self.mllama_lm = encoder == "mllama"
        if self.mllama_lm:  # the image side is the tile tower; the language tower is loaded beside it below
            encoder = "mllama_tiles"
        elif lm_geometry is not None or prompt_ids is not None:
            raise ValueError("lm_geometry= and prompt_ids= belong to encoder='mllama'")
        if encoder not in ("vit_b16", "vit", "clip", "siglip_vit", "dinov2", "mllama_tiles"):
            raise ValueError("encoder must be 'vit_b16' (BASELINE.json's re-scoped ViT-B/16), 'vit' (the ViT/16 family: ViT-S, -B and -L widths), "
                             "'clip' (a CLIP ViT/16 image tower of that family), 'siglip_vit' (a SigLIP ViT/16 image tower of that family), "
                             "'dinov2' (a DINOv2 ViT/14 image tower) or 'mllama_tiles' (the checkpoint's own vision-tower geometry)")
        if encoder == "siglip_vit" and pool != "cls":
            raise ValueError(f"pool = {pool!r}: encoder='siglip_vit' pools with the tower's attention-pooling head; supported: the default")
        if pool in ("mean", "cls+mean") and encoder not in ("vit", "dinov2"):
            raise ValueError(f"pool = {pool!r}: encoder={encoder!r} pools one token row, or for itself (CLIP's projection, the tile tower's features); "
                             "supported: 'mean' and 'cls+mean' with encoder='vit' and encoder='dinov2'")
        # this class spells the tower "siglip_vit" (the bare name "siglip" stays a refused encoder here); below it is checkpoint.py's "siglip"
        if encoder == "siglip_vit":
            encoder = "siglip"
        if encoder == "vit_b16" and geometry is not None:
            raise ValueError("encoder='vit_b16' is ViT-B/16 only; pass encoder='vit' with geometry=")
        self.resize_rule = check_resize_rule(resize_rule, encoder)
        # a caller's engine carries its own weights
        source = "weights" if engine is not None else resolve_model_source(model_name, weights, allow_synthetic)
        if source == "checkpoint":
            self.checkpoint = read_checkpoint(model_name, encoder, resize_rule)
        elif self.resize_rule == "checkpoint":
            raise MmeError(f"resize_rule = 'checkpoint' reads preprocessor_config.json of a checkpoint directory; model_name = {model_name!r} is "
                           "none, or weights= / engine= was given (supported: a local checkpoint directory, or a ResizeSpec that names the rule)")
        if engine is not None:
            dev_list = [engine.device]
        elif devices is not None:  # explicit device indices (may repeat: several contexts on one GPU)
            dev_list = [int(d) for d in devices]
        elif isinstance(device, int):
            dev_list = [device]
        elif isinstance(device, str) and device not in ("cuda",):
            if not device.startswith("cuda"):
                raise MmeError(f"device={device!r}: this engine is HIP only (no CPU fallback)")
            dev_list = [int(device.split(":")[1]) if ":" in device else 0]
        elif "LOCAL_RANK" in os.environ:  # one process per GPU under torchrun / bench.py
            dev_list = [int(os.environ["LOCAL_RANK"])]
        else:  # embedder.py:54-65: gpu_count of the visible GPUs, all of them by default
            if not torch.cuda.is_available():
                raise MmeError("no GPU visible to torch; the embed/compare path is HIP only (no CPU fallback)")
            available = torch.cuda.device_count()
            n = available if gpu_count is None else max(1, min(int(gpu_count), available))
            logger.info(f"Using {n} of {available} available GPUs")
            dev_list = list(range(n))
        if not dev_list:
            raise MmeError("no device selected")
        self.gpu_count = len(dev_list)
        self.devices = [f"cuda:{d}" for d in dev_list]
        self.device = torch.device(self.devices[0])
        self.encoder = encoder
        rec = ENCODER_TABLE[encoder]
        if engine is not None:
            self.engines = [engine]
        elif self.checkpoint is not None:
            ck = self.checkpoint
            self.engines = []
            for d in dev_list:  # read once, loaded into every context
                e = Engine(d)
                # only the tile tower takes a geometry beside its checkpoint: the save point of the intermediate states is not in the file
                getattr(e, rec.loader + "_checkpoint")(ck, *([geometry] if encoder == "mllama_tiles" else []))
                if ck.image_mean is not None:
                    e.set_normalisation(ck.image_mean, ck.image_std)
                self.engines.append(e)
        else:
            if geometry is None and (weights is None or rec.infer_geometry is None):  # a caller's dict is sized by its tensors where that can be read
                geometry = rec.geometry
            w = weights if weights is not None else rec.make_weights(seed + rec.seed_offset, geometry)
            self.engines = []
            for d in dev_list:  # one context (weights + workspace) per device, as embedder.py:73-82
                e = Engine(d)
                getattr(e, rec.loader)(w, geom=geometry)
                self.engines.append(e)
        self.engine = self.engines[0]
        if self.resize_rule == "checkpoint":
            self.resize_rule = self.checkpoint.resize_spec
        if isinstance(self.resize_rule, ResizeSpec):
            for e in self.engines:
                e.set_resize_spec(self.resize_rule)
        elif resize_rule is not None:
            for e in self.engines:
                e.set_resize_rule(self.resize_rule)
        # a caller's engine keeps its rule under None; this object reports what the engine runs
        self.resize_rule, self.resize_spec = self.engine.resize_rule, self.engine.resize_spec
        if chunk:
            for e in self.engines:
                e.set_chunk(chunk)
        if prune_last_layer is None:  # default: on for the contexts this object created, a caller's engine stays as it is
            prune_last_layer = engine is None
        if prune_last_layer and encoder in ("vit_b16", "vit", "clip", "dinov2"):
            # only the pooled token's row of the last layer is computed past its attention (mme_set_forward_pruning): callers of
            # this class only ever receive pooled vectors, and those are bit-identical, 6 % sooner.  The benchmark's headline
            # drives the Engine directly and times the whole forward; `prune_last_layer=False` restores that here.
            for e in self.engines:
                e.set_forward_pruning(True)
        if pool not in ("cls", "last", "mean", "cls+mean"):
            raise ValueError("pool must be 'cls' or 'last' (one token row), or 'mean' or 'cls+mean' (the mean of the patch rows a crop covers; "
                             "encoder='vit' and 'dinov2')")
        self.pool = pool
        if pool in ("mean", "cls+mean"):
            for e in self.engines:  # every context pools alike: the covered patches of each crop, [class row | mean] under "cls+mean"
                e.set_pooling(pool)
        # the last token: 196 of the 197 at patch 16 (the same at every width), 49 of the 50 at patch 32, 256 of the 257 at patch 14
        # (SigLIP: the library ignores the token, the head pools; so do the mean modes)
        self.pool_token = (196 if encoder == "mllama_tiles" else self.engine.vit_geometry().seq_len - 1) if pool == "last" else 0
        # width of the returned vectors: the ViT's hidden size, the tile tower's concatenated features
        self.embed_dim = int(getattr(self.engine, "tile_features", TILE_VIT.output_dim)) if encoder == "mllama_tiles" else int(self.engine.embed_dim)
        self._tokenizer = tokenizer
        if self.mllama_lm:  # may replace self._tokenizer by the directory's own
            self._load_mllama_lm(engine is None, weights, seed, lm_geometry, prompt_ids, tokenizer)
        self._seed = seed
        self._text_source = text_tower  # None: look in model_name on first use; False: never
        self._text_dir = None           # where a default tokenizer is looked for
        self._text_loaded = False
        if text_tower is not None and text_tower is not False:
            self._load_text_tower()

    MLLAMA_PROMPT = "<|image|><|begin_of_text|> Represent the given image."  # the reference's prompt (embedder.py:108); the tokenizer puts its BOS in front

    def _load_mllama_lm(self, own_engines, weights, seed, lm_geometry, prompt_ids, tokenizer):
        """The language tower of encoder='mllama' into every context this object made (a caller's engine brings its own), the
        prompt of the image path as ids, and `embed_dim` = the text hidden size."""
        from .weights import MLLAMA_LM_11B, make_mllama_lm_weights

        self._tokenizer = tokenizer
        if own_engines and self.checkpoint is not None:  # one directory holds both towers and the projector
            from .checkpoint import read_checkpoint

            self.lm_checkpoint = read_checkpoint(self.model_name, "mllama_text")
            if self.lm_checkpoint.geometry.vision_output_dim != int(getattr(self.engine, "tile_features", TILE_VIT.output_dim)):
                raise MmeError(f"{self.model_name}: vision_output_dim = {self.lm_checkpoint.geometry.vision_output_dim}, but the tile tower puts out "
                               f"{self.engine.tile_features} features")
            for e in self.engines:
                e.load_mllama_lm_checkpoint(self.lm_checkpoint)
            if tokenizer is None and any(os.path.exists(os.path.join(self.model_name, f)) for f in ("tokenizer.json", "tokenizer.model")):
                from transformers import AutoTokenizer  # the directory's own tokenizer files, never fetched

                self._tokenizer = AutoTokenizer.from_pretrained(self.model_name, local_files_only=True)
        elif own_engines:
            geom = lm_geometry or MLLAMA_LM_11B
            features = int(getattr(self.engine, "tile_features", TILE_VIT.output_dim))
            if geom.vision_output_dim != features:
                raise ValueError(f"lm_geometry.vision_output_dim = {geom.vision_output_dim}; supported: the tile tower's output width {features}")
            w = make_mllama_lm_weights(seed + 6, geom)
            for e in self.engines:
                e.load_mllama_lm(w, geom)
        info = self.engine.mllama_lm_info()
        if not info["loaded"]:
            raise MmeError("encoder='mllama': the engine holds no language tower (Engine.load_mllama_lm)")
        self._mllama_info = info
        self.embed_dim = int(info["hidden_size"])
        if prompt_ids is None:  # the reference's prompt, which only a tokenizer can turn into ids
            prompt_ids = self.MLLAMA_PROMPT
        self.prompt_ids = self._mllama_ids(prompt_ids, "prompt_ids")
        if info["image_token_id"] not in self.prompt_ids:
            raise ValueError(f"prompt_ids hold no image token (id {info['image_token_id']}): the image path needs one")

    def _mllama_ids(self, item, what):
        """A str through `tokenizer=`, or a 1-D sequence of token ids -> list[int], checked against the tower's table and 128 positions."""
        if isinstance(item, str):
            tok = getattr(self, "_tokenizer", None)
            if tok is None:
                raise ValueError(f"{what}: a str needs tokenizer= (a callable str -> list[int] or a transformers tokenizer); without one pass "
                                 "prompt_ids= / token ids")
            out = tok(item)
            item = out["input_ids"] if isinstance(out, dict) or hasattr(out, "input_ids") else out
        a = np.asarray(item)
        if a.ndim != 1 or a.dtype.kind not in "iu" or not 1 <= a.shape[0] <= 128:
            raise MmeError(f"{what}: token ids must be a 1-D integer sequence of 1..128 ids, got {a.dtype} {tuple(a.shape)}")
        rows = self._mllama_info["vocab_size"] + 8
        if a.min() < 0 or a.max() >= rows:
            raise MmeError(f"{what}: ids outside 0..{rows - 1}")
        return [int(v) for v in a]

    def _mllama_text(self, text):
        single = isinstance(text, str)
        if not single:
            a = text if isinstance(text, np.ndarray) else None
            if a is None and isinstance(text, (list, tuple)) and len(text) and not isinstance(text[0], (str, list, tuple, np.ndarray)):
                a = np.asarray(text)
            single = a is not None and a.ndim == 1
        items = [text] if single else list(text)
        if not items:
            return []
        rows = [self._mllama_ids(it, "get_text_embeddings") for it in items]
        S = max(len(r) for r in rows)
        ids = np.zeros((len(rows), S), dtype=np.int32)  # right padding: under the causal mask it reaches no attended row
        for i, r in enumerate(rows):
            ids[i, : len(r)] = r
        e32, _ = self.engines[0].mllama_lm_forward(ids, np.array([len(r) for r in rows], dtype=np.int32), want_bf16=False)
        out = [[float(v) for v in r] for r in e32.cpu().numpy()]
        return out[0] if single else out

    # -- device-resident API -------------------------------------------------------------------
    def pack(self, arrays, device=None):
        """list of uint8[h,w,3] -> (pix CUDA tensor, offs int64[n], hw int32[n,2])."""
        t = self.torch
        device = self.device if device is None else device
        n = len(arrays)
        hw = np.array([a.shape[:2] for a in arrays], dtype=np.int32).reshape(n, 2)
        offs, sizes, total = packed_layout(hw)
        host = t.empty(total, dtype=t.uint8, pin_memory=t.cuda.is_available())
        hv = host.numpy()
        for a, o, s in zip(arrays, offs, sizes):
            hv[o : o + s] = a.reshape(-1)
        return host.to(device, non_blocking=True), offs, hw

    def embed_packed(self, pix, offs, hw, want_f32=True, want_bf16=True):
        """Packed crops already in HBM -> (f32 [n, embed_dim], bf16 [n, embed_dim]) CUDA tensors."""
        return self.engine.embed(pix, offs, hw, self.pool_token, want_f32=want_f32, want_bf16=want_bf16)

    def embed_uniform(self, crops):
        """uint8 CUDA tensor [n,224,224,3] (the synthetic C2/C4 workload) -> (f32, bf16)."""
        n = crops.shape[0]
        per = int(np.prod(crops.shape[1:]))
        offs = np.arange(n, dtype=np.int64) * per
        hw = np.tile(np.array([[crops.shape[1], crops.shape[2]]], dtype=np.int32), (n, 1))
        return self.engine.embed(crops.reshape(-1), offs, hw, self.pool_token)

    def process_images(self, images, tile=560, max_tiles=4):
        """What `self.processors[i](images=[image], return_tensors="pt")` hands the reference's model
        (embedder.py:117-121), for a batch of single-image samples, computed on the GPU (K1 multi-tile):
        {"pixel_values": f32 CUDA [B, 1, max_tiles, 3, tile, tile], "aspect_ratio_ids": int64 [B, 1],
         "aspect_ratio_mask": int64 [B, 1, max_tiles], "num_tiles": [[n], ...]} -- bit-exact with transformers'
        MllamaImageProcessorPil at the checkpoint geometry (tile 560, <= 4 tiles) when the engine's mean/std are
        the checkpoint's (the CLIP values by default)."""
        arrays = [_load_rgb(item) for item in images]
        pix, offs, hw = self.pack(arrays)
        pv, ids, mask, nt = self.engine.preprocess_tiles(pix, offs, hw, tile, max_tiles)
        return {"pixel_values": pv[:, None], "aspect_ratio_ids": ids[:, None], "aspect_ratio_mask": mask[:, None, :],
                "num_tiles": [[int(v)] for v in nt]}

    # -- reference surface ------------------------------------------------------------------------
    def _pipe_state(self, dev_idx):
        """Per-context staging of the host <-> device pipeline of `_embed_list`: two slots, each a pinned input buffer and its
        device twin (grown on demand, kept), a copy stream for the H2D, the result ring with the D2H stream (the two copy
        engines run side by side) and the events that order them against the compute stream.  The host-logic tests drive
        the pipeline with a stand-in engine and no device: streams and events are then staging's no-ops."""
        st = self.__dict__.setdefault("_pipes", {})  # atomic: contexts are driven from one thread each, concurrently
        if dev_idx not in st:
            dev = self.torch.device(self.devices[dev_idx])
            with on(dev):
                st[dev_idx] = {
                    "in_stream": new_stream(dev), "ring": ResultRing(dev, 256),
                    "pin": [None, None], "dev": [None, None], "pinned": dev.type == "cuda",
                    "used": [False, False],  # a slot's events mean something once it has been staged, in ANY earlier call
                    "ev_in": [new_event(dev), new_event(dev)], "ev_done": [new_event(dev), new_event(dev)],
                }
        return st[dev_idx]

    def _stage_group(self, pipe, slot, arrays, device):
        """Pack decoded crops into the slot's pinned buffer (`packed_layout`, as `pack`) and start their H2D copy on the
        input stream.  Returns (device pixels, offs, hw, cap jobs).  The slot's previous occupants are out of the way: the caller
        acquired the slot after the consumer recorded `ev_done[slot]` (the pass that read the device twin)."""
        t = self.torch
        n = len(arrays)
        hw = np.array([a.shape[:2] for a in arrays], dtype=np.int32).reshape(n, 2)
        offs, sizes, total = packed_layout(hw)
        # An oversized item (_Oversized): `offs` / `hw` point at its CAPPED image, a hole the consumer thread fills on the
        # device; its raw pixels ride behind the crops (host and device buffer), its workspace behind those (device only).
        jobs, srcs = [], []  # jobs: (raw offset, h, w, new_h, new_w, capped offset, workspace offset, workspace bytes)
        for k, a in enumerate(arrays):
            if isinstance(a, _Oversized):
                at = (total + 255) // 256 * 256
                srcs.append((at, a.raw))
                jobs.append([at, a.raw.shape[0], a.raw.shape[1], a.new_h, a.new_w, int(offs[k]), 0, a.work])
                total = at + int(a.raw.nbytes)
        total_dev = total
        for job in jobs:
            job[6] = (total_dev + 255) // 256 * 256
            total_dev = job[6] + job[7]
        first_use = not pipe["used"][slot]  # per pipe state, not per call: a call that left through an exception may have
        pipe["used"][slot] = True           # work in flight on the buffers the next call finds
        if pipe["pin"][slot] is None or pipe["pin"][slot].numel() < total or pipe["dev"][slot].numel() < total_dev:
            if not first_use:  # the buffers about to be dropped may still be read: by the last H2D, by the last pass
                pipe["ev_in"][slot].synchronize()
                pipe["ev_done"][slot].synchronize()
            pipe["pin"][slot] = t.empty(max(total, 1 << 20), dtype=t.uint8, pin_memory=pipe["pinned"])
            pipe["dev"][slot] = t.empty(max(total_dev, 1 << 20), dtype=t.uint8, device=device)
        elif not first_use:
            pipe["ev_in"][slot].synchronize()  # the last H2D out of this pinned buffer has finished (long ago)
        hv = pipe["pin"][slot].numpy()
        for at, raw in srcs:
            hv[at : at + raw.nbytes] = raw.reshape(-1)

        def copy_range(lo, hi):  # large numpy copies release the GIL: a few threads fill the buffer side by side
            for k in range(lo, hi):
                if not isinstance(arrays[k], _Oversized):
                    o, sz = int(offs[k]), int(sizes[k])
                    hv[o : o + sz] = arrays[k].reshape(-1)

        nbytes = int(sizes.sum())
        workers = min(4, os.cpu_count() or 1, max(1, nbytes >> 26))  # one thread per 64 MB, at most four
        if workers > 1:
            cuts = np.searchsorted(np.cumsum(sizes), np.linspace(0, nbytes, workers + 1)[1:-1]).tolist()
            bounds = [0] + [int(c) for c in cuts] + [n]
            with ThreadPoolExecutor(max_workers=workers) as pool:
                list(pool.map(lambda ab: copy_range(*ab), zip(bounds[:-1], bounds[1:])))
        else:
            copy_range(0, n)
        with on(device, pipe["in_stream"]):
            if not first_use:
                pipe["in_stream"].wait_event(pipe["ev_done"][slot])  # the pass that read the device twin has run
            pipe["dev"][slot][:total].copy_(pipe["pin"][slot][:total], non_blocking=True)
            pipe["ev_in"][slot].record(pipe["in_stream"])
        return pipe["dev"][slot][:total_dev], offs, hw, jobs

    @staticmethod
    def _run_cap_jobs(engine, pix, jobs):
        """The device cap of a staged group's oversized items, on the calling thread's current stream: raw pixels ->
        LANCZOS -> the hole `offs` points at, each through its own workspace inside `pix`.  The caller is the thread that
        runs the pass over `pix` next (mme_lanczos_resize uses no buffer of the context)."""
        for at, h, w, nh, nw, dst, work, work_bytes in jobs:
            engine.lanczos_resize(pix[at : at + h * w * 3].view(h, w, 3), nh, nw, out=pix[dst : dst + nh * nw * 3], work=pix[work : work + work_bytes])

    def _embed_list(self, dev_idx, items, step, as_array=False, sink=None):
        """One context's share of a call: [(index, item)] -> [(index, list[float] | None)] (embedder.py:86-139); float32
        ndarray rows under `as_array`; `sink`: see `_pass`.

        The items go through in bounded groups -- at most `step` (16 x batch_size) crops and GROUP_BYTES of packed pixels per
        `mme_embed` call -- each decoded, packed and embedded inside its own try/except: a failure (an unreadable
        file, an out-of-memory MmeError) voids only what it touched.

        The reference runs open -> processor -> forward -> `.cpu().tolist()` strictly in series per image
        (embedder.py:104-137).  Here the host side of group g + 1 (decode on a thread pool, packing into a pinned
        buffer, H2D on a copy stream) runs on a producer thread UNDER the device pass of group g, and the D2H of group
        g plus the float lists of group g - 1 behind it: two staging slots, three streams, events between them
        (staging.Stage and staging.ResultRing)."""
        if self.encoder == "mllama_tiles":
            return self._embed_list_serial(dev_idx, items, step)
        engine = self.engines[dev_idx]
        device = self.torch.device(self.devices[dev_idx])
        pipe = self._pipe_state(dev_idx)
        results = []

        def produce(stage):  # decode, host copies and H2D on the input stream: no engine call on this thread
            g = 0
            with on(device):
                for failed, groups in _decoded_groups(items, step, self.GROUP_BYTES):
                    if failed:
                        stage.put(("failed", failed))
                    for group in groups:
                        slot = g & 1
                        if not stage.acquire(slot):
                            return
                        try:
                            staged = self._stage_group(pipe, slot, [a for _, a in group], device)
                        except Exception as e:  # embedder.py:223-224
                            logger.error(f"Error in batch processing: {e}")
                            stage.release(slot)
                            stage.put(("failed", [i for i, _ in group]))
                            continue
                        stage.put(("group", slot, [i for i, _ in group], staged))
                        g += 1

        def finalize(idx, rows):
            if as_array:
                rows = list(rows.copy())  # float32 rows (get_image_embeddings(as_array=True))
            else:
                # embedder.py:132 `.cpu().tolist()`.  In slices: one tolist() of a whole group holds the GIL for tens of
                # milliseconds, during which the producer thread cannot even start its next (GIL-free) buffer copy
                rows = [row for c0 in range(0, len(rows), 64) for row in rows[c0 : c0 + 64].tolist()]
            results.extend(zip(idx, rows))

        ring = pipe["ring"]
        ring.start(finalize)
        with Stage(f"mme-stage-{dev_idx}", produce, 2, device, logger) as stage, on(device):
            compute = current_stream(device)
            for msg in iter(stage.get, None):
                if msg[0] == "failed":
                    results.extend((i, None) for i in msg[1])
                    continue
                _, slot, idx, (pix, offs, hw, jobs) = msg
                try:
                    compute.wait_event(pipe["ev_in"][slot])
                    self._run_cap_jobs(engine, pix, jobs)  # this thread, the compute stream: ordered before the pass
                    e32 = self._pass(engine, pix, offs, hw, idx, sink)
                except Exception as e:  # embedder.py:223-224
                    logger.error(f"Error in batch processing: {e}")
                    e32 = None
                pipe["ev_done"][slot].record(compute)
                stage.release(slot)  # the producer may refill the slot: its H2D waits for ev_done on the device
                if e32 is None:
                    results.extend((i, None) for i in idx)
                else:  # D2H behind the pass; the float lists of the previous group under this group's device pass
                    ring.submit(e32, pipe["ev_done"][slot], idx)
            ring.finish()
        return results

    def _pass(self, engine, pix, offs, hw, idx, sink=None):
        """The device pass of one packed group -> f32 [n, embed_dim].  With a `sink` (get_patch_embeddings) the same pass also returns
        the patch-token rows (mme_embed_tokens; its pooled rows are mme_embed's bit for bit), which go to rows `idx` of the sink."""
        if sink is None:
            e32, _ = engine.embed(pix, offs, hw, self.pool_token, want_bf16=False)
            return e32
        t = self.torch
        tokens, e32, _ = engine.embed_tokens(pix, offs, hw, self.pool_token, want_bf16=False)
        rows = t.as_tensor(list(idx), dtype=t.int64, device=tokens.device)
        if sink.device == tokens.device:
            sink.index_copy_(0, rows, tokens)
        else:  # another context's share: through that device's stream, then ordered into the sink's
            t.cuda.current_stream(tokens.device).synchronize()
            sink.index_copy_(0, rows.to(sink.device), tokens.to(sink.device))
        return e32

    def _embed_list_serial(self, dev_idx, items, step):
        """The unpipelined form of `_embed_list` for the tile-ViT option: decode -> stage -> cap -> pass -> lists per group of at
        most TILE_GROUP_CROPS crops, all on the calling thread, through the first staging slot of the context."""
        engine = self.engines[dev_idx]
        device = self.torch.device(self.devices[dev_idx])
        pipe = self._pipe_state(dev_idx)
        results = []
        with on(device):
            compute = current_stream(device)
            for failed, groups in _decoded_groups(items, min(step, self.TILE_GROUP_CROPS), self.GROUP_BYTES):
                results.extend((i, None) for i in failed)
                for group in groups:
                    idx = [i for i, _ in group]
                    try:
                        pix, offs, hw, jobs = self._stage_group(pipe, 0, [a for _, a in group], device)
                        try:
                            compute.wait_event(pipe["ev_in"][0])
                            self._run_cap_jobs(engine, pix, jobs)
                            # processor (K1 multi-tile) + vision tower, class token of tile 0 (7680-d)
                            pv, ids, _, nt = engine.preprocess_tiles(pix, offs, hw, 560, 4)
                            if getattr(self, "mllama_lm", False):  # ... + projector + language tower under the prompt: the reference's 4096-d vector
                                e32, _ = engine.mllama_embed(pv, ids, nt, np.tile(np.asarray(self.prompt_ids, dtype=np.int32), (len(idx), 1)), want_bf16=False)
                            else:
                                _, e32, _ = engine.tile_vit_forward(pv, ids, nt, want_bf16=False)
                        finally:
                            pipe["ev_done"][0].record(compute)  # the next group's H2D into the slot waits for this
                        results.extend(zip(idx, e32.cpu().tolist()))
                    except Exception as e:  # embedder.py:223-224
                        logger.error(f"Error in batch processing: {e}")
                        results.extend((i, None) for i in idx)
        return results

    def get_image_embeddings(self, image_paths, is_query=False, batch_size=config.BATCH_SIZE, *, as_array=False):
        """embedder.py:141-226: order-preserving list of float lists with None holes.

        `as_array=True` (an addition to the reference's signature) returns (float32 [n, D] ndarray, bool [n] mask of
        the rows that were embedded) instead: building n x D Python floats costs more host time than the device pass.

        Item i goes to context i % n_devices (:191-203) and every context works through its share on its own
        thread (:208-224); a single query image takes the first context without the pool (:158-185).
        `batch_size` keeps the reference's meaning "images per GPU per batch", except that a device pass here
        carries 16 of the reference's one-image forwards per unit of it (256 crops at the default 16)."""
        return self._embed_all(image_paths, is_query, batch_size, bool(as_array), None)

    def _embed_all(self, image_paths, is_query, batch_size, as_array, sink):
        """get_image_embeddings; with a `sink` the passes also leave their patch tokens there (get_patch_embeddings, `_pass`)."""
        if not image_paths:
            return (np.zeros((0, getattr(self, "embed_dim", config.EMBED_DIM)), dtype=np.float32), np.zeros(0, dtype=bool)) if as_array else []
        step = 16 * max(1, int(batch_size))
        embeddings = [None] * len(image_paths)
        n_dev = len(self.engines)
        if n_dev == 1 or (len(image_paths) == 1 and is_query):
            shares = [list(enumerate(image_paths))]
        else:
            shares = [[(i, p) for i, p in enumerate(image_paths) if i % n_dev == d] for d in range(n_dev)]
        if len(shares) == 1:
            done = [self._embed_list(0, shares[0], step, as_array, sink)]
        else:
            with ThreadPoolExecutor(max_workers=n_dev) as pool:
                done = list(pool.map(lambda d: self._embed_list(d, shares[d], step, as_array, sink), range(n_dev)))
        for part in done:
            for i, row in part:
                embeddings[i] = row
        if as_array:
            ok = np.array([row is not None for row in embeddings], dtype=bool)
            width = next((len(row) for row in embeddings if row is not None), getattr(self, "embed_dim", config.EMBED_DIM))
            arr = np.zeros((len(embeddings), width), dtype=np.float32)
            for i, row in enumerate(embeddings):
                if row is not None:
                    arr[i] = row
            return arr, ok
        return embeddings

    def get_patch_embeddings(self, images, out=None, batch_size=config.BATCH_SIZE):
        """get_image_embeddings that also keeps the patch tokens of every crop: returns (vectors, tokens).

        `vectors` is exactly what get_image_embeddings returns for the same input (float lists, None holes included).  `tokens` is a
        bfloat16 CUDA tensor [n, ntok, hidden] in input order on the first context's device -- the caller's `out` if given -- whose
        row (i, t) is the tower's final LayerNorm of patch token t of crop i, L2-normalised: ntok = 196 (ViT/16, CLIP/16, SigLIP), 49
        (patch 32) or 256 (DINOv2); the class token is left out.  A failed item's block is zeros.

        Size: n * ntok * hidden * 2 bytes -- 301 KB per ViT-B/16 crop, 19.7 GB at 65 536 crops; pass `out` to place it, or call in
        slices.  Not available for encoder="mllama_tiles" (the tile tower's 4 x 1601 tokens of 1280 are another object)."""
        if self.encoder == "mllama_tiles":
            raise NotImplementedError("get_patch_embeddings: encoder 'mllama_tiles'; supported: the single-tile image towers "
                                      "(vit, clip, siglip_vit, dinov2)")
        t = self.torch
        n = len(images)
        g = self.engine.vit_geometry()
        shape = (n, g.num_patches, g.hidden_size)
        dev = t.device(self.devices[0])
        if out is None:
            out = t.zeros(shape, dtype=t.bfloat16, device=dev)
        else:
            if out.dtype != t.bfloat16 or not out.is_contiguous() or not out.is_cuda or tuple(out.shape) != shape:
                raise ValueError(f"get_patch_embeddings: `out` must be a contiguous bfloat16 CUDA tensor {list(shape)}")
            out.zero_()
        t.cuda.synchronize(out.device)  # the zeros are in place before any context's stream writes a block
        try:
            vectors = self._embed_all(images, False, batch_size, False, out)
        finally:
            for d in self.devices:
                t.cuda.synchronize(t.device(d))
        return vectors, out

    def embed(self, region):
        """north_star `embed(region) -> vec`: one crop -> float32[embed_dim] (raises on failure)."""
        out = self.get_image_embeddings([region], is_query=True)
        if out[0] is None:
            raise MmeError("embed(region) failed; see log")
        return np.asarray(out[0], dtype=np.float32)

    # -- text queries (embedder.py:228-254) ------------------------------------------------------------------
    _NO_TOWER = ("text embeddings need a CLIP text tower: construct RegionEmbedder(..., text_tower=True | a checkpoint directory | a weight "
                 "dict), or name a checkpoint directory that holds one (a whole CLIPModel); the mmE5 language tower stays out of scope")

    def _load_text_tower(self):
        """Loads the tower `text_tower=` named into the first engine (SigLIP's 64-token tower under encoder='siglip_vit', whose width
        is checked against the image side; else CLIP's); NotImplementedError when there is none to load."""
        from .checkpoint import read_checkpoint
        from .encoders import ENCODER_TABLE

        src = getattr(self, "_text_source", False)
        eng = self.engines[0]
        if self.encoder == "dinov2":
            raise NotImplementedError("text embeddings: a DINOv2 tower is trained on images alone and has no text tower; " + self._NO_TOWER)
        # (a CLIP text tower embeds into another space than a SigLIP image tower)
        siglip = self.encoder == "siglip"
        kind, no_tower = ("siglip_text", self._NO_SIGLIP_TOWER) if siglip else ("clip_text", self._NO_TOWER)
        rec = ENCODER_TABLE[kind]
        if src is False:
            raise NotImplementedError(no_tower)
        if isinstance(src, dict):
            if siglip:
                self._check_siglip_text_width(rec.infer_geometry(src).projection_size, "the weight dict")
            getattr(eng, rec.loader)(src)
        elif isinstance(src, (str, os.PathLike)) or self.checkpoint is not None:
            own = not isinstance(src, (str, os.PathLike))  # None or True beside a checkpoint directory: its own text half
            directory = self.model_name if own else src
            try:
                ck = read_checkpoint(directory, kind)
            except MmeError as e:
                if own and src is None:  # a vision-only directory
                    raise NotImplementedError(f"{no_tower} ({e})") from e
                raise
            if siglip:
                self._check_siglip_text_width(ck.geometry.projection_size, os.fspath(directory))
            getattr(eng, rec.loader + "_checkpoint")(ck)
            self._text_dir = os.fspath(directory)
        elif src is True:  # seeded, in the space (SigLIP: at the width) of the seeded image side
            geom = rec.beside(int(self.embed_dim))
            getattr(eng, rec.loader)(rec.make_weights(self._seed + 2, geom), geom)
        else:
            raise NotImplementedError(no_tower)
        self._text_loaded = True

    _NO_SIGLIP_TOWER = ("text embeddings under encoder='siglip_vit' need a SigLIP text tower: construct RegionEmbedder(..., text_tower=True | a "
                        "checkpoint directory | a weight dict), or name a checkpoint directory that holds text_model.* (a whole SiglipModel)")

    def _check_siglip_text_width(self, projection: int, where: str):
        if int(projection) != int(self.embed_dim):
            raise MmeError(f"text_tower: {where}: projection_size = {projection}; supported: {self.embed_dim}, the embed_dim of the loaded "
                           "SigLIP image tower (the two towers must embed into one space)")

    def _text_layout(self):
        """(tokens per sequence, id that right-pads a short sequence) of the first engine's text tower: 77 and the eos_token_id
        of a CLIP tower, 64 and the pad_token_id of a SigLIP tower."""
        eng = self.engines[0]
        geometry = getattr(eng, "text_geometry", None)
        if geometry is None:  # an engine that knows CLIP towers only
            return 77, eng.text_info()["eos_token_id"]
        g = geometry()
        return g["tokens"] or 77, g["pad_token_id"]

    def _tokenize(self, text: str) -> list:
        """str -> token ids through `tokenizer=` or the lazily loaded tokenizer of the tower's directory (CLIPTokenizer; under a
        SigLIP tower whatever AutoTokenizer reads from the local files), padded to the tower's token count."""
        tok = getattr(self, "_tokenizer", None)
        T = self._text_layout()[0]
        if tok is None and T != 77:
            d = getattr(self, "_text_dir", None)
            hint = "pass tokenizer= (a callable str -> list[int] or a transformers tokenizer); token ids (a sequence of ints) are accepted as they are"
            if d is None:
                raise MmeError(f"get_text_embeddings: no tokenizer for a str: {hint}")
            try:
                from transformers import AutoTokenizer

                tok = AutoTokenizer.from_pretrained(d, local_files_only=True)  # nothing is ever fetched
            except Exception as e:  # noqa: BLE001 - missing files, or a tokenizer library this machine does not have
                raise MmeError(f"get_text_embeddings: the libraries here read no SigLIP tokenizer from {d!r}: {e}; {hint}") from e
            self._tokenizer = tok
        if tok is None:
            d = getattr(self, "_text_dir", None)
            hint = "pass tokenizer= (a callable str -> list[int] or a transformers tokenizer); token ids (a sequence of ints) are accepted as they are"
            if d is None:
                raise MmeError(f"get_text_embeddings: no tokenizer for a str: {hint}")
            have = lambda *names: all(os.path.exists(os.path.join(d, n)) for n in names)  # noqa: E731
            if not (have("vocab.json", "merges.txt") or have("tokenizer.json")):
                raise MmeError(f"get_text_embeddings: {d!r} holds no CLIP tokenizer files (vocab.json + merges.txt, or tokenizer.json): {hint}")
            try:
                from transformers import CLIPTokenizer
            except ImportError as e:
                raise MmeError(f"get_text_embeddings: transformers is not installed, so {d!r} cannot be tokenized: {hint}") from e
            try:
                tok = CLIPTokenizer.from_pretrained(d, local_files_only=True)  # nothing is ever fetched
            except Exception as e:  # noqa: BLE001 - whatever the reader raises for missing or broken files
                raise MmeError(f"get_text_embeddings: {d!r} holds no usable CLIP tokenizer files (vocab.json, merges.txt): {e}; {hint}") from e
            self._tokenizer = tok
        if hasattr(tok, "pad_token_id") or hasattr(tok, "encode"):  # a transformers tokenizer
            ids = tok(text, padding="max_length", max_length=T, truncation=True)["input_ids"]
        else:
            ids = tok(text)
        return [int(v) for v in ids]

    def _text_ids(self, item) -> np.ndarray:
        """One query -> int32[77] (int32[64] under a SigLIP tower): a str through the tokenizer, ids right-padded with the
        tower's eos_token_id (SigLIP: its pad_token_id)."""
        ids = self._tokenize(item) if isinstance(item, str) else item
        a = np.asarray(ids)
        if a.ndim != 1 or a.dtype.kind not in "iu":
            raise MmeError(f"get_text_embeddings: token ids must be a 1-D integer sequence, got {a.dtype} {tuple(a.shape)}")
        T, pad = self._text_layout()
        if a.shape[0] > T:
            raise MmeError(f"get_text_embeddings: {a.shape[0]} token ids; supported: at most {T}")
        row = np.full(T, pad, dtype=np.int64)
        row[: a.shape[0]] = a
        return row

    def get_text_embeddings(self, text):
        """A str, or a 1-D sequence / array of token ids -> list[float] of `text_embed_dim`, unit length; a list of str, or
        a 2-D int array -> a list of such vectors.  Raises on failure, as the reference's does (embedder.py:228-254).
        NotImplementedError without a text tower."""
        engines = getattr(self, "engines", None)
        if engines and getattr(self, "mllama_lm", False):  # the language tower without an image: the cross layers are skipped
            return self._mllama_text(text)
        if not engines or getattr(self, "_text_source", False) is False:
            raise NotImplementedError(self._NO_TOWER)
        if not getattr(self, "_text_loaded", False):
            self._load_text_tower()
        single = isinstance(text, str)
        if not single:
            a = text if isinstance(text, np.ndarray) else None
            if a is None and isinstance(text, (list, tuple)) and len(text) and not isinstance(text[0], (str, list, tuple, np.ndarray)):
                a = np.asarray(text)
            single = a is not None and a.ndim == 1
        items = [text] if single else list(text)
        if not items:
            return []
        ids = np.stack([self._text_ids(it) for it in items])
        e32, _ = engines[0].text_forward(ids, want_f32=True, want_bf16=False)
        rows = e32.cpu().numpy()
        out = [[float(v) for v in r] for r in rows]
        return out[0] if single else out

    def siglip_probabilities(self, texts_or_vectors, image_vectors) -> np.ndarray:
        """SigLIP's zero-shot scores of m texts against N image vectors: sigmoid(exp(logit_scale) cos + logit_bias), f32 [m, N]
        (SiglipModel.forward's logits_per_text under a sigmoid).  `texts_or_vectors`: what `get_text_embeddings` takes (a list
        of str or of id sequences, or one of either), or a float array [m, embed_dim] of unit vectors; `image_vectors`: a float
        array [N, embed_dim] of unit vectors (`get_image_embeddings`).  The cosine block is the engine's bf16 GEMM, the scores
        its kernel.  MmeError unless the loaded text tower is SigLIP's and came with logit_scale and logit_bias."""
        engines = getattr(self, "engines", None)
        if not engines or getattr(self, "_text_source", False) is False:
            raise NotImplementedError(self._NO_SIGLIP_TOWER)
        if not getattr(self, "_text_loaded", False):
            self._load_text_tower()
        eng, t = engines[0], self.torch
        a = texts_or_vectors if isinstance(texts_or_vectors, np.ndarray) else None
        if a is not None and a.dtype.kind == "f":
            tv = np.atleast_2d(a)
        else:
            rows = self.get_text_embeddings(texts_or_vectors)
            tv = np.atleast_2d(np.asarray(rows, dtype=np.float32))
        iv = np.atleast_2d(np.asarray(image_vectors, dtype=np.float32))
        if tv.ndim != 2 or iv.ndim != 2 or tv.shape[1] != iv.shape[1]:
            raise MmeError(f"siglip_probabilities: text vectors {tuple(tv.shape)} against image vectors {tuple(iv.shape)}")
        if tv.shape[1] % 64:
            raise MmeError(f"siglip_probabilities: vectors of {tv.shape[1]} values; supported: a multiple of 64")
        dev = t.device("cuda", eng.device)
        with t.cuda.device(dev):
            tb = t.from_numpy(np.ascontiguousarray(tv, dtype=np.float32)).to(dev).to(t.bfloat16).contiguous()
            ib = t.from_numpy(np.ascontiguousarray(iv)).to(dev).to(t.bfloat16).contiguous()
            cos = eng.cosine(tb, ib)
            p = eng.siglip_scores(cos, out=cos)
            return p.cpu().numpy()

    @property
    def text_embed_dim(self) -> int:
        """Width of the vectors `get_text_embeddings` returns; 0 while no text tower is loaded."""
        return int(self.engines[0].text_embed_dim)


# the reference's class name, so `from embedder import MmE5MllamaEmbedder` call sites port 1:1
MmE5MllamaEmbedder = RegionEmbedder
