"""sl.RenderPass / sl.RenderPassResult (reference include/stillleben/render_pass.h:35-153,
python/src/py_render_pass.cpp:81-279)."""

from . import _abi
from ._context import engine, require_context


class RenderPassResult:
    """Accessors return the dtypes/shapes of the reference (py_render_pass.cpp:20-69):
    rgb u8[H,W,4]; class/instance int16[H,W,1] (R16UI bits reinterpreted); coordinates f32[H,W,3];
    depth f32[H,W]; coordDepth/normals/cam_coordinates f32[H,W,4]; vertex_indices int32[H,W,3];
    barycentric_coeffs f32[H,W,3]."""

    def __init__(self):
        require_context()
        self._buffers = None
        self._index = 0

    def _get(self, name):
        if self._buffers is None:
            raise RuntimeError("RenderPassResult is empty: render something first")
        t = getattr(self._buffers, name)
        if t is None:
            raise RuntimeError("output '%s' was not requested for this render" % name)
        t = t[self._index]
        # fresh tensor per call, like extract() (py_magnum.cpp:17-46)
        return t.clone() if require_context().cuda_outputs else t.cpu()

    def rgb(self):
        return self._get("rgb")

    def class_index(self):
        return self._get("cls")

    def instance_index(self):
        return self._get("instance")

    def coordinates(self):
        return self._get("coord")[:, :, 0:3]

    def depth(self):
        return self._get("coord")[:, :, 3]

    def coordDepth(self):  # noqa: N802 (reference name)
        return self._get("coord")

    def normals(self):
        return self._get("normals")

    def vertex_indices(self):
        return self._get("vertex_idx")[:, :, 0:3]

    def barycentric_coeffs(self):
        return self._get("bary")[:, :, 0:3]

    def cam_coordinates(self):
        return self._get("cam_coord")

    def object_stats(self):
        """Per-object visibility statistics of the rendered scene (sl.ObjectStats, tensors [S] / [S, 4]; slot i = instance
        index i), computed when RenderPass.object_stats_enabled was set for the render.  Raises RuntimeError otherwise."""
        if self._buffers is None:
            raise RuntimeError("RenderPassResult is empty: render something first")
        st = self._buffers.object_stats
        if st is None:
            raise RuntimeError("the last render did not compute object statistics (set RenderPass.object_stats_enabled)")
        cuda = require_context().cuda_outputs
        return st[self._index].map(lambda t: t.clone() if cuda else t.cpu())

    def object_masks(self):
        """Per-object masks of the rendered scene (sl.ObjectMasks, the single scene's view: dense(kind, slots=...), rle(i, kind),
        rles(kind); slot i = instance index i), computed when RenderPass.object_masks_enabled was set for the render.  Raises
        RuntimeError otherwise.  The bit tiles and run lengths stay on the device; `.stats` follows the other accessors."""
        if self._buffers is None:
            raise RuntimeError("RenderPassResult is empty: render something first")
        om = self._buffers.object_masks
        if om is None:
            raise RuntimeError("the last render did not compute object masks (set RenderPass.object_masks_enabled)")
        cuda = require_context().cuda_outputs
        one = om[self._index]
        one.stats = one.stats.map(lambda t: t.clone() if cuda else t.cpu())
        return one


class RenderPass:
    def __init__(self, shading="pbr"):
        require_context()
        if shading not in ("pbr", "phong", "flat"):
            raise ValueError("unknown shading type specified")
        self._shading = shading  # stored, never read by the render path (quirk q2)
        self.ssao_enabled = True  # render_pass.h:150
        self.object_stats_enabled = False   # additive: per-object visibility statistics (RenderPassResult.object_stats())
        self.object_masks_enabled = False   # additive: per-object masks (RenderPassResult.object_masks(); the statistics come along)
        self._result = RenderPassResult()
        self._buffers = None

    def render(self, scene, result=None, depth_peel=None, predicate=None):
        """With object_stats_enabled or object_masks_enabled, a `depth_peel` render raises ValueError: a peeled layer has no
        single whole silhouette."""
        if (self.object_stats_enabled or self.object_masks_enabled) and depth_peel is not None:
            raise ValueError("object statistics / masks cannot be combined with depth_peel: a peeled layer has no single whole silhouette")
        res = result if result is not None else self._result
        peel = None
        if depth_peel is not None:
            peel = depth_peel._buffers.coord[depth_peel._index:depth_peel._index + 1].contiguous()
        own = res._buffers if (res._buffers is not None and res._buffers.B == 1 and res is not depth_peel) else None
        res._buffers = engine().render([scene], _abi.OUT_ALL, ssao=self.ssao_enabled, shadows=True,
                                       depth_peel=peel, predicate=predicate, buffers=own, object_stats=self.object_stats_enabled,
                                       object_masks=self.object_masks_enabled)
        res._index = 0
        return res

    def render_batch(self, scenes, outputs=_abi.OUT_ALL, shadows=True):
        """Additive API: renders many scenes in one launch sequence; returns the batched
        [B,H,W,C] buffers (device tensors)."""
        return engine().render(list(scenes), outputs, ssao=self.ssao_enabled, shadows=shadows)
