"""orbslam3lib_amd -- MI355X-native ORB front-end (Python mirror of the reference interface).

The compute path is liborbgpu.so (HIP kernels for gfx950 behind the C ABI in
include/orbgpu.h).  This module mirrors the reference's operator surface so the parity tests
read like the reference's own call sites:

  ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
      cpp/include/ORBextractor_old.h:51-59; operator() :56-59; getters :62-84; mvImagePyramid :86
  ORBmatcher.DescriptorDistance(a, b)        cpp/include/ORBmatcher.h:44
  BFMatcher(NORM_HAMMING).knnMatch(q, t, 2)  cpp/src/Frame.cc:45,1227

There is no CPU fallback: if liborbgpu.so or a gfx950 device is missing, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

__all__ = ["ORBextractor", "ORBmatcher", "BFMatcher", "BatchExtractor", "KEYPOINT_DTYPE", "MAP_POINT_DTYPE",
           "LAST_POINT_DTYPE", "TRACK_POSE_DTYPE", "RELOC_POINT_DTYPE", "RELOC_POSE_DTYPE", "TRIANG_POINT_DTYPE",
           "TRIANG_PAIR_DTYPE", "FUSE_POINT_DTYPE", "predict_scale_table",
           "OrbGpuError", "load_library", "LIB_PATH"]

HERE = os.path.dirname(os.path.abspath(__file__))
# ORBGPU_LIB names another build of the same library (measurement variants under tools/)
LIB_PATH = os.environ.get("ORBGPU_LIB") or os.path.join(HERE, "liborbgpu.so")

# orbgpu_map_point (60 B): the MapPoint state ORBmatcher::SearchByProjection reads
MAP_POINT_DTYPE = np.dtype([("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"), ("view_cos", "<f4"),
                            ("depth", "<f4"), ("level", "<i4"), ("flags", "<i4"), ("desc", "u1", (32,)),
                            ("proj_yr", "<f4"), ("view_cos_r", "<f4"), ("level_r", "<i4")])
MP_IN_VIEW, MP_BAD, MP_HAS_OBS, MP_IN_VIEW_R = 1, 2, 4, 8

# orbgpu_last_point (56 B): what the motion-model SearchByProjection reads of a last-frame point;
# orbgpu_track_pose (96 B): CurrentFrame.GetPose() and LastFrame.GetPose(), row-major
LAST_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("angle", "<f4"), ("octave", "<i4"), ("flags", "<i4"),
                             ("desc", "u1", (32,))])
TRACK_POSE_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("Rlw", "<f4", (9,)), ("tlw", "<f4", (3,))])
LP_VALID = 1  # ORBGPU_LP_VALID (MP_HAS_OBS is shared)
# orbgpu_track_rig (80 B): the left KannalaBrandt8 camera (fx fy cx cy k0..k3) and Frame::mTrl, row-major
TRACK_RIG_DTYPE = np.dtype([("cam_left", "<f4", (8,)), ("Rrl", "<f4", (9,)), ("trl", "<f4", (3,))])
# orbgpu_bow_point (44 B): a keyframe keypoint for search_by_bow
BOW_POINT_DTYPE = np.dtype([("desc", "u1", (32,)), ("angle", "<f4"), ("node", "<i4"), ("flags", "<i4")])
BOW_HAS_POINT = 1  # ORBGPU_BOW_HAS_POINT
BOW_MAX_POINTS = 8192  # ORBGPU_BOW_MAX_POINTS
# orbgpu_bowkf_point: a keypoint of keyframe 2 for search_by_bow_kf, the same 44 bytes; ORBGPU_BOWKF_*: the
# decision a keypoint of keyframe 1 ended with (ORBmatcher.cc:766-906)
BOWKF_POINT_DTYPE = BOW_POINT_DTYPE
BOWKF_HAS_POINT = 1  # ORBGPU_BOWKF_HAS_POINT
(BOWKF_NO_NODE, BOWKF_NODE_NOT_COMMON, BOWKF_NO_MAP_POINT, BOWKF_NO_CANDIDATE, BOWKF_NOT_BELOW_TH_LOW,
 BOWKF_RATIO_FAILED, BOWKF_MATCHED, BOWKF_ROTATION_REJECTED) = range(1, 9)
# orbgpu_triang_point (56 B): a keypoint of keyframe 2 for search_for_triangulation; orbgpu_triang_pair
# (44 B): the pair's F12 (row-major) and the epipole in keyframe 2
TRIANG_POINT_DTYPE = np.dtype([("desc", "u1", (32,)), ("x", "<f4"), ("y", "<f4"), ("angle", "<f4"),
                               ("octave", "<i4"), ("node", "<i4"), ("flags", "<i4")])
TRIANG_PAIR_DTYPE = np.dtype([("F12", "<f4", (9,)), ("ep", "<f4", (2,))])
TRI_HAS_POINT, TRI_STEREO = 1, 2  # ORBGPU_TRI_HAS_POINT, ORBGPU_TRI_STEREO
# orbgpu_reloc_point (60 B): a keyframe's map point for reloc_by_projection; orbgpu_reloc_pose (60 B):
# CurrentFrame.GetPose(), row-major, and its camera centre Tcw.inverse().translation()
RELOC_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("angle", "<f4"), ("min_distance", "<f4"),
                              ("max_distance", "<f4"), ("flags", "<i4"), ("desc", "u1", (32,))])
RELOC_POSE_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("Ow", "<f4", (3,))])
RP_VALID = 1  # ORBGPU_RP_VALID
# orbgpu_fuse_point (68 B): a map point for fuse; the poses are RELOC_POSE_DTYPE rows
FUSE_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"),
                             ("max_distance", "<f4"), ("flags", "<i4"), ("desc", "u1", (32,))])
FP_VALID = 1  # ORBGPU_FP_VALID
FUSE_MAX_POINTS = 65536  # ORBGPU_FUSE_MAX_POINTS
# ORBGPU_FUSE_*: the decision a point ended with (the reference's count_* counters, ORBmatcher.cc:1183)
(FUSE_SKIPPED, FUSE_NEG_DEPTH, FUSE_NOT_IN_IMAGE, FUSE_DISTANCE, FUSE_NORMAL, FUSE_EMPTY_WINDOW, FUSE_ABOVE_TH_LOW,
 FUSE_FUSED) = range(1, 9)
# ORBGPU_SIM3_*: the decision a point of sim3_search_by_projection ended with (1 to 6 are the FUSE_* values),
# and the projection of each overload (ORBmatcher.cc:428: Pinhole::project; :535: the invz form)
(SIM3_SKIPPED, SIM3_NEG_DEPTH, SIM3_NOT_IN_IMAGE, SIM3_DISTANCE, SIM3_NORMAL, SIM3_EMPTY_WINDOW, SIM3_NOT_MATCHED,
 SIM3_MATCHED) = range(1, 9)
SIM3_PROJECT_DIV, SIM3_PROJECT_INVZ = 0, 1

# cv::KeyPoint layout (28 B)
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

EXPORTED = [
    "orbgpu_create", "orbgpu_destroy", "orbgpu_get_scale_tables", "orbgpu_extract",
    "orbgpu_extract_stereo", "orbgpu_upload_images", "orbgpu_device_input", "orbgpu_run_batch",
    "orbgpu_download_result", "orbgpu_download_counts", "orbgpu_synchronize",
    "orbgpu_get_pyramid_level", "orbgpu_get_level_keypoints", "orbgpu_match_knn2",
    "orbgpu_match_stereo_batch", "orbgpu_download_matches", "orbgpu_descriptor_distance",
    "orbgpu_stereo_matches_batch", "orbgpu_download_stereo", "orbgpu_candidate_counts",
    "orbgpu_image_bounds", "orbgpu_undistort_grid_batch", "orbgpu_download_grid",
    "orbgpu_device_sbs_input", "orbgpu_upload_sbs", "orbgpu_ingest_sbs", "orbgpu_pack_soa",
    "orbgpu_download_soa", "orbgpu_download_matches16", "orbgpu_extract_features",
    "orbgpu_search_by_projection_batch", "orbgpu_search_by_projection_stereo",
    "orbgpu_download_projection_matches", "orbgpu_upload_images_async", "orbgpu_host_alloc",
    "orbgpu_host_free", "orbgpu_export_descriptors", "orbgpu_match_knn2_device",
    "orbgpu_set_profiling", "orbgpu_num_stages", "orbgpu_stage_name", "orbgpu_stage_times",
    "orbgpu_reset_stage_times", "orbgpu_last_error", "orbgpu_abi_version",
    "orbgpu_fisheye_stereo_batch", "orbgpu_download_fisheye", "orbgpu_run_batch_match",
    "orbgpu_diagnostic_knobs", "orbgpu_ingest_images", "orbgpu_export_batch_bytes", "orbgpu_export_batch",
    "orbgpu_get_device", "orbgpu_track_by_projection_batch", "orbgpu_download_track_matches",
    "orbgpu_track_by_projection_stereo", "orbgpu_search_for_initialization_batch",
    "orbgpu_download_initialization_matches", "orbgpu_search_by_bow_batch", "orbgpu_download_bow_matches",
    "orbgpu_reloc_by_projection_batch", "orbgpu_download_reloc_matches", "orbgpu_predict_scale_table",
    "orbgpu_search_for_triangulation_batch", "orbgpu_download_triangulation_matches",
    "orbgpu_fuse_batch", "orbgpu_download_fuse_matches",
    "orbgpu_sim3_search_by_projection_batch", "orbgpu_download_sim3_matches", "orbgpu_sim3_replay_stats",
    "orbgpu_search_by_bow_kf_batch", "orbgpu_download_bow_kf_matches",
]

DEVICE_CURRENT = -1  # ORBGPU_DEVICE_CURRENT: the calling thread's current HIP device


class KB8Rig(C.Structure):
    """orbgpu_kb8_rig: the two KannalaBrandt8 cameras and Frame::mRlr / mtlr."""
    _fields_ = [("cam_left", C.c_float * 8), ("cam_right", C.c_float * 8), ("precision_left", C.c_float),
                ("precision_right", C.c_float), ("R12", C.c_float * 9), ("t12", C.c_float * 3)]

    @classmethod
    def make(cls, cam_left, cam_right, R12=None, t12=(0.0, 0.0, 0.0), precision_left=1e-6,
             precision_right=1e-6):
        r = cls()
        r.cam_left[:] = [float(v) for v in cam_left]
        r.cam_right[:] = [float(v) for v in cam_right]
        r.precision_left, r.precision_right = precision_left, precision_right
        R = np.eye(3, dtype=np.float32) if R12 is None else np.asarray(R12, np.float32).reshape(9)
        r.R12[:] = [float(v) for v in np.ravel(R)]
        r.t12[:] = [float(v) for v in t12]
        return r

    def as_dict(self):
        return dict(cam_left=list(self.cam_left), cam_right=list(self.cam_right),
                    precision_left=self.precision_left, precision_right=self.precision_right,
                    R12=np.array(list(self.R12), np.float32).reshape(3, 3), t12=list(self.t12))


class OrbGpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("orbgpu error %d: %s" % (code, msg))
        self.code = code


class _Params(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32)]


_lib = None


def load_library(path: str = LIB_PATH):
    """Load liborbgpu.so (raises if it has not been built -- no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise OrbGpuError(-6, "liborbgpu.so not built (run `make` or __graft_entry__.build())")
    lib = C.CDLL(path)
    lib.orbgpu_last_error.restype = C.c_char_p
    lib.orbgpu_stage_name.restype = C.c_char_p
    lib.orbgpu_device_input.restype = C.c_void_p
    lib.orbgpu_device_input.argtypes = [C.c_void_p]
    lib.orbgpu_device_sbs_input.restype = C.c_void_p
    lib.orbgpu_device_sbs_input.argtypes = [C.c_void_p]
    lib.orbgpu_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
    lib.orbgpu_host_free.argtypes = [C.c_void_p]
    lib.orbgpu_diagnostic_knobs.argtypes = [C.c_char_p, C.c_size_t]
    lib.orbgpu_export_descriptors.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                              C.POINTER(C.c_int), C.c_void_p]
    lib.orbgpu_match_knn2_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + \
        [C.c_void_p] * 5
    lib.orbgpu_ingest_images.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.orbgpu_export_batch_bytes.restype = C.c_size_t
    lib.orbgpu_export_batch_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.orbgpu_export_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                        C.POINTER(C.c_size_t), C.c_void_p]
    lib.orbgpu_get_device.argtypes = [C.c_void_p]
    for name in ("orbgpu_destroy", "orbgpu_synchronize", "orbgpu_set_profiling",
                 "orbgpu_reset_stage_times"):
        getattr(lib, name).argtypes = [C.c_void_p] + ([C.c_int] if name == "orbgpu_set_profiling" else [])
    _lib = lib
    return lib


def hip_function(name: str):
    """A HIP runtime entry point (e.g. "hipMemcpy2D") from the runtime liborbgpu.so is bound to.
    ctypes looks the name up with dlsym on the library's handle, which searches liborbgpu.so and
    then its dependencies in load order, i.e. the libamdhip64 it actually mapped (torch's bundled
    copy when torch was imported first) -- no soname is hard-coded.  Test / bench plumbing."""
    return getattr(load_library(), name)


def diagnostic_knobs() -> dict:
    """The measurement knobs liborbgpu.so honours right now (orbgpu_diagnostic_knobs): empty
    unless ORBGPU_DIAGNOSTICS=1 is set beside them."""
    buf = C.create_string_buffer(4096)
    load_library().orbgpu_diagnostic_knobs(buf, len(buf))
    txt = buf.value.decode()
    return dict(kv.split("=", 1) for kv in txt.split(";")) if txt else {}


def predict_scale_table(scale_factor, nlevels) -> np.ndarray:
    """orbgpu_predict_scale_table: float32 [nlevels - 1], entry n the largest ratio = mfMaxDistance /
    dist3D whose MapPoint::PredictScale (host logf) is at most n.  The clamped level of a ratio is the
    number of entries below it.  Host computation: no device is needed."""
    lib = load_library()
    t = np.zeros(max(int(nlevels) - 1, 0), np.float32)
    _check(lib.orbgpu_predict_scale_table(C.c_float(scale_factor), int(nlevels), _p(t) if len(t) else None))
    return t


def _check(code):
    if code < 0:
        raise OrbGpuError(code, _lib.orbgpu_last_error().decode())
    return code


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


_COUNT_STATUS = {-5: "device workspace overflow (octree)", -2: "context output capacity exceeded"}


def decode_export(buf, n_images, n_pairs):
    """The packed orbgpu_export_batch layout (include/orbgpu.h) -> ([(kps, desc, mono)] per image,
    [(idx1, dist1, idx2, dist2)] per pair).  Raises OrbGpuError on a status word in a count."""
    b = np.ascontiguousarray(buf, dtype=np.uint8).reshape(-1)
    hdr = 4 * (2 * n_images + n_pairs)
    if b.size < hdr:
        raise OrbGpuError(-2, "export buffer shorter than its header")
    h = b[:hdr].view(np.int32)
    counts, mono, nq = h[:n_images], h[n_images:2 * n_images], h[2 * n_images:]
    for c in list(counts) + list(nq):
        if c < 0:
            code = int(c) if int(c) in _COUNT_STATUS else -2
            raise OrbGpuError(code, _COUNT_STATUS.get(int(c), "negative row count in export"))
    if b.size < hdr + 60 * int(counts.sum()) + 16 * int(nq.sum()):
        raise OrbGpuError(-2, "export buffer shorter than its counts say")
    o = hdr
    images = []
    for i in range(n_images):
        n = int(counts[i])
        kps = b[o:o + 28 * n].copy().view(KEYPOINT_DTYPE); o += 28 * n
        desc = b[o:o + 32 * n].copy().reshape(n, 32); o += 32 * n
        images.append((kps, desc, int(mono[i])))
    pairs = []
    for p in range(n_pairs):
        n = int(nq[p])
        m = b[o:o + 16 * n].copy().view(np.int32).reshape(4, n); o += 16 * n
        pairs.append(tuple(m[k] for k in range(4)))
    return images, pairs


def encode_export(images, pairs):
    """Host restatement of the packed layout (what orbgpu_export_batch writes) from per-image
    (kps, desc, mono) and per-pair (idx1, dist1, idx2, dist2): the CPU stand-ins' export."""
    parts = [np.array([len(k) for k, _, _ in images], np.int32), np.array([m for _, _, m in images], np.int32),
             np.array([len(p[0]) for p in pairs], np.int32)]
    for k, d, _ in images:
        parts.append(np.ascontiguousarray(k, KEYPOINT_DTYPE).view(np.uint8).reshape(-1))
        parts.append(np.ascontiguousarray(d, np.uint8).reshape(-1))
    for p in pairs:
        parts.append(np.stack([np.asarray(a, np.int32) for a in p]).reshape(-1))
    return np.concatenate([x.view(np.uint8).reshape(-1) for x in parts])


class _Context:
    def __init__(self, nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, device, max_width,
                 max_height, max_images):
        lib = load_library()
        self.params = _Params(int(nfeatures), float(scaleFactor), int(nlevels), int(iniThFAST),
                              int(minThFAST))
        self.handle = C.c_void_p()
        _check(lib.orbgpu_create(C.byref(self.params), int(device), int(max_width),
                                 int(max_height), int(max_images), C.byref(self.handle)))
        self.nlevels = int(nlevels)
        self.max_images = int(max_images)

    def device(self):
        """The HIP ordinal the context runs on (orbgpu_get_device)."""
        return _check(_lib.orbgpu_get_device(self.handle))

    def close(self):
        if self.handle:
            _lib.orbgpu_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ORBextractor:
    """ORB_SLAM3::ORBextractor on the GPU (cpp/src/ORBextractor_old.cc:411-1191).

    __call__(image, mask=None, vLappingArea=(0, 0)) -> (keypoints, descriptors, monoIndex)
      keypoints: structured array with cv::KeyPoint fields; descriptors: uint8 [N, 32];
      monoIndex: number of keypoints outside the lapping area (written first).
      Returns (empty, None, -1) for an empty image, like the reference (:1092-1093).
    """

    def __init__(self, nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, device=0,
                 max_width=1920, max_height=1080, max_images=2):
        self.nfeatures = int(nfeatures)
        self.scaleFactor = float(scaleFactor)
        self.nlevels = int(nlevels)
        self.iniThFAST = int(iniThFAST)
        self.minThFAST = int(minThFAST)
        self._ctx = _Context(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, device,
                             max_width, max_height, max_images)
        L = self.nlevels
        self.mvScaleFactor = np.zeros(L, np.float32)
        self.mvInvScaleFactor = np.zeros(L, np.float32)
        self.mvLevelSigma2 = np.zeros(L, np.float32)
        self.mvInvLevelSigma2 = np.zeros(L, np.float32)
        self.mnFeaturesPerLevel = np.zeros(L, np.int32)
        _check(_lib.orbgpu_get_scale_tables(self._ctx.handle, _p(self.mvScaleFactor),
                                            _p(self.mvInvScaleFactor), _p(self.mvLevelSigma2),
                                            _p(self.mvInvLevelSigma2), _p(self.mnFeaturesPerLevel)))
        self._cap = 4 * max(self.nfeatures, 1) * 2 + 64 * L + 4096
        self._last_n_images = 0

    # getters (ORBextractor_old.h:62-84)
    def GetLevels(self):
        return self.nlevels

    def GetScaleFactor(self):
        return self.scaleFactor

    def GetScaleFactors(self):
        return self.mvScaleFactor.tolist()

    def GetInverseScaleFactors(self):
        return self.mvInvScaleFactor.tolist()

    def GetScaleSigmaSquares(self):
        return self.mvLevelSigma2.tolist()

    def GetInverseScaleSigmaSquares(self):
        return self.mvInvLevelSigma2.tolist()

    def __call__(self, image, mask=None, vLappingArea=(0, 0)):
        img = np.asarray(image)
        if img.size == 0:
            return np.zeros(0, KEYPOINT_DTYPE), None, -1
        if img.dtype != np.uint8 or img.ndim != 2:
            raise OrbGpuError(-3, "image must be CV_8UC1 (2-D uint8)")  # assert :1096
        img = np.ascontiguousarray(img)
        h, w = img.shape
        kps = np.zeros(self._cap, KEYPOINT_DTYPE)
        desc = np.zeros((self._cap, 32), np.uint8)
        n, mono = C.c_int(0), C.c_int(0)
        _check(_lib.orbgpu_extract(self._ctx.handle, _p(img), w, h, w, int(vLappingArea[0]),
                                   int(vLappingArea[1]), _p(kps), _p(desc), self._cap,
                                   C.byref(n), C.byref(mono)))
        self._last_n_images = 1
        return kps[:n.value], (desc[:n.value] if n.value else None), mono.value

    def extract_stereo(self, left, right, lapLeft=(0, 0), lapRight=(0, 0)):
        """Stereo operator() (cpp/include/ORBextractor.h:52-57): both eyes in one device pass."""
        left = np.ascontiguousarray(left, dtype=np.uint8)
        right = np.ascontiguousarray(right, dtype=np.uint8)
        h, w = left.shape
        out = []
        bufs = [(np.zeros(self._cap, KEYPOINT_DTYPE), np.zeros((self._cap, 32), np.uint8),
                 C.c_int(0), C.c_int(0)) for _ in range(2)]
        la = (C.c_int * 2)(*lapLeft)
        ra = (C.c_int * 2)(*lapRight)
        (kl, dl, nl, ml), (kr, dr, nr, mr) = bufs
        _check(_lib.orbgpu_extract_stereo(self._ctx.handle, _p(left), _p(right), w, h, w, la, ra,
                                          _p(kl), _p(dl), C.byref(nl), C.byref(ml), _p(kr), _p(dr),
                                          C.byref(nr), C.byref(mr), self._cap))
        self._last_n_images = 2
        for k, d, n, m in bufs:
            out.append((k[:n.value], d[:n.value], m.value))
        return out

    @property
    def mvImagePyramid(self):
        """Levels of the last extracted image (public member, ORBextractor_old.h:86)."""
        return [self.pyramid_level(0, l) for l in range(self.nlevels)]

    def pyramid_level(self, image, level, blurred=False):
        w, h = C.c_int(0), C.c_int(0)
        _check(_lib.orbgpu_get_pyramid_level(self._ctx.handle, image, level, int(blurred), None, 0,
                                             C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.uint8)
        _check(_lib.orbgpu_get_pyramid_level(self._ctx.handle, image, level, int(blurred), _p(out),
                                             w.value, None, None))
        return out

    def level_keypoints(self, image=0):
        """Per-level keypoints (level coords, octree order, with angle) + descriptors."""
        kps = np.zeros(self._cap, KEYPOINT_DTYPE)
        desc = np.zeros((self._cap, 32), np.uint8)
        cnt = np.zeros(self.nlevels, np.int32)
        _check(_lib.orbgpu_get_level_keypoints(self._ctx.handle, image, _p(kps), _p(desc), self._cap,
                                               _p(cnt)))
        out, off = [], 0
        for c in cnt.tolist():
            out.append((kps[off:off + c], desc[off:off + c]))
            off += c
        return out


class ORBmatcher:
    @staticmethod
    def DescriptorDistance(a, b):
        """Hamming distance of two 32-byte descriptors (cpp/src/ORBmatcher.cc:2107-2123)."""
        lib = load_library()
        a = np.ascontiguousarray(a, dtype=np.uint8).reshape(32)
        b = np.ascontiguousarray(b, dtype=np.uint8).reshape(32)
        return lib.orbgpu_descriptor_distance(_p(a), _p(b))


class BFMatcher:
    """cv::BFMatcher(NORM_HAMMING) with knnMatch(k=2) on the GPU."""

    def __init__(self, extractor: ORBextractor):
        self._ctx = extractor._ctx

    def knnMatch(self, query, train, k=2):
        """Returns (idx1, dist1, idx2, dist2) int32 arrays; idx = -1 where absent."""
        if k != 2:
            raise OrbGpuError(-3, "only k=2 is implemented (the reference uses k=2)")
        q = np.ascontiguousarray(query, dtype=np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(train, dtype=np.uint8).reshape(-1, 32)
        nq = q.shape[0]
        out = [np.zeros(nq, np.int32) for _ in range(4)]
        _check(_lib.orbgpu_match_knn2(self._ctx.handle, _p(q), nq, _p(t), t.shape[0],
                                      *[_p(o) for o in out]))
        return tuple(out)


class BatchExtractor:
    """Device-resident batch path (the throughput path used by bench.py).

    upload(images[n,h,w]) -> run(laps) -> results stay in HBM; match_stereo() pairs 2p/2p+1.
    """

    device_resident = True  # results live in HBM (dist.cross_camera_match_device)

    def __init__(self, nfeatures=2000, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7,
                 device=0, width=640, height=480, max_images=128):
        self.ctx = _Context(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, device, width,
                            height, max_images)
        self.width, self.height = int(width), int(height)
        self.n = 0
        self._staged = None  # (n, h, w) of the batch upload_async staged for the next run()
        self._pinned = []

    def close(self):
        """Frees the pinned host buffers of pinned() and the device context."""
        self.free_pinned()
        self.ctx.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, images):
        imgs = np.ascontiguousarray(images, dtype=np.uint8)
        n, h, w = imgs.shape
        _check(_lib.orbgpu_upload_images(self.ctx.handle, _p(imgs), n, w, h, w))
        self.n, self.height, self.width = n, h, w
        self._staged = None  # the synchronous upload replaces a staged one (orbgpu_upload_images)
        _check(_lib.orbgpu_synchronize(self.ctx.handle))

    def knn_match(self, query, train):
        """BFMatcher(NORM_HAMMING).knnMatch(query, train, 2) on this context's device, host arrays
        in and out: (idx1, dist1, idx2, dist2) int32."""
        q = np.ascontiguousarray(query, dtype=np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(train, dtype=np.uint8).reshape(-1, 32)
        out = [np.zeros(q.shape[0], np.int32) for _ in range(4)]
        _check(_lib.orbgpu_match_knn2(self.ctx.handle, _p(q), q.shape[0], _p(t), t.shape[0], *[_p(o) for o in out]))
        return tuple(out)

    def export_descriptors(self, image, device_ptr, cap_rows, row0=0, stream=None):
        """Rows [row0, n) of image's descriptors into device memory (device-to-device);
        returns the row count."""
        n = C.c_int(0)
        _check(_lib.orbgpu_export_descriptors(self.ctx.handle, int(image), int(row0), C.c_void_p(device_ptr),
                                              int(cap_rows), C.byref(n), C.c_void_p(stream) if stream else None))
        return n.value

    def match_knn2_device(self, d_query, nq, d_train, nt, d_out, stream=None):
        """kNN2 on device buffers; d_out: device int32 [4, nq] (idx1, dist1, idx2, dist2)."""
        _check(_lib.orbgpu_match_knn2_device(self.ctx.handle, C.c_void_p(d_query), int(nq), C.c_void_p(d_train),
                                             int(nt), C.c_void_p(d_out), C.c_void_p(d_out + 4 * nq),
                                             C.c_void_p(d_out + 8 * nq), C.c_void_p(d_out + 12 * nq),
                                             C.c_void_p(stream) if stream else None))

    def ingest_images(self, device_ptr, n, stride=None, stream=None):
        """n images of this context's size already in device memory (rows of `stride` bytes,
        e.g. a collective's receive buffer) -> the input buffer, device to device
        (orbgpu_ingest_images); the next run() / run_match() reads them."""
        _check(_lib.orbgpu_ingest_images(self.ctx.handle, C.c_void_p(device_ptr), int(n), self.width, self.height,
                                         int(stride or self.width), C.c_void_p(stream) if stream else None))
        self.n = int(n)
        self._staged = None

    def export_batch_bytes(self, n_images, n_pairs):
        """The largest orbgpu_export_batch layout (every image at the context's row capacity)."""
        return int(_lib.orbgpu_export_batch_bytes(self.ctx.handle, int(n_images), int(n_pairs)))

    def export_batch_size(self, n_images, n_pairs, stream=None):
        """The exact size of the packed orbgpu_export_batch layout of the last batch (waits for it)."""
        used = C.c_size_t(0)
        _check(_lib.orbgpu_export_batch(self.ctx.handle, int(n_images), int(n_pairs), None, 0, C.byref(used),
                                        C.c_void_p(stream) if stream else None))
        return used.value

    def export_batch(self, device_ptr, n_images, n_pairs, nbytes, stream=None):
        """The last batch's produced rows of images [0, n_images) and pairs [0, n_pairs) packed into
        one device buffer (orbgpu_export_batch, device to device); returns the bytes written."""
        used = C.c_size_t(0)
        _check(_lib.orbgpu_export_batch(self.ctx.handle, int(n_images), int(n_pairs), C.c_void_p(device_ptr),
                                        int(nbytes), C.byref(used), C.c_void_p(stream) if stream else None))
        return used.value

    @staticmethod
    def decode_export(buf, n_images, n_pairs):
        """Host view of an orbgpu_export_batch buffer (uint8 array, trailing padding allowed): per
        image (keypoints in the cv::KeyPoint layout, descriptors [n, 32], mono index) and per pair
        (idx1, dist1, idx2, dist2) over the pair's query rows -- what result() / matches() return.
        A negative count is a device status word (-5 octree workspace overflow, -2 capacity), not
        rows: raised as OrbGpuError, as every download path does."""
        return decode_export(buf, n_images, n_pairs)

    def upload_async(self, images):
        """Stage the NEXT batch (orbgpu_upload_images_async): the copy runs beside the current
        batch's kernels; the next run() reads it.  `images` should come from pinned()."""
        imgs = np.ascontiguousarray(images, dtype=np.uint8)
        n, h, w = imgs.shape
        _check(_lib.orbgpu_upload_images_async(self.ctx.handle, _p(imgs), n, w, h, w))
        # the current batch keeps its size until run() switches to the staged one: counts(),
        # match_stereo() etc. issued before that still refer to the current batch
        self._staged = (n, h, w)

    def pinned(self, shape):
        """A uint8 numpy array over page-locked host memory.  The memory is freed by free_pinned()
        or close() (or when the extractor is collected); the array must not be used after that."""
        nbytes = int(np.prod(shape))
        ptr = C.c_void_p()
        _check(_lib.orbgpu_host_alloc(nbytes, C.byref(ptr)))
        self._pinned.append(ptr)
        buf = (C.c_uint8 * nbytes).from_address(ptr.value)
        return np.frombuffer(buf, np.uint8).reshape(shape)

    def free_pinned(self):
        """Frees every pinned() buffer (after the staged uploads that read them have landed)."""
        if self._pinned and self.ctx.handle:
            _check(_lib.orbgpu_synchronize(self.ctx.handle))
        for ptr in self._pinned:
            _lib.orbgpu_host_free(ptr)
        self._pinned = []

    def run(self, laps=None, stream=None):
        if self._staged is not None:  # the batch upload_async staged becomes the current one
            self.n, self.height, self.width = self._staged
            self._staged = None
        n = self.n
        lp = None
        if laps is not None:
            lp = np.ascontiguousarray(laps, dtype=np.int32).reshape(n, 2)
        _check(_lib.orbgpu_run_batch(self.ctx.handle, n, self.width, self.height,
                                     _p(lp) if lp is not None else None,
                                     C.c_void_p(stream) if stream else None))

    def run_match(self, laps=None, stereo_rows_only=False, stream=None):
        """run() then match_stereo() over every pair as one submission when the batch is one
        captured graph (orbgpu_run_batch_match; the latency shape)."""
        if self._staged is not None:
            self.n, self.height, self.width = self._staged
            self._staged = None
        n = self.n
        lp = None
        if laps is not None:
            lp = np.ascontiguousarray(laps, dtype=np.int32).reshape(n, 2)
        _check(_lib.orbgpu_run_batch_match(self.ctx.handle, n, self.width, self.height,
                                           _p(lp) if lp is not None else None, int(stereo_rows_only),
                                           C.c_void_p(stream) if stream else None))

    def match_stereo(self, stereo_rows_only=False, stream=None):
        _check(_lib.orbgpu_match_stereo_batch(self.ctx.handle, self.n // 2, int(stereo_rows_only),
                                              C.c_void_p(stream) if stream else None))

    def synchronize(self):
        _check(_lib.orbgpu_synchronize(self.ctx.handle))

    def counts(self):
        n = np.zeros(self.n, np.int32)
        m = np.zeros(self.n, np.int32)
        _check(_lib.orbgpu_download_counts(self.ctx.handle, self.n, _p(n), _p(m)))
        return n, m

    def candidate_counts(self):
        """Keys that entered DistributeOctTree per image (all levels) in the last run()."""
        c = np.zeros(self.n, np.int32)
        _check(_lib.orbgpu_candidate_counts(self.ctx.handle, self.n, _p(c)))
        return c

    def result(self, i, cap=65536):
        kps = np.zeros(cap, KEYPOINT_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n, m = C.c_int(0), C.c_int(0)
        _check(_lib.orbgpu_download_result(self.ctx.handle, i, _p(kps), _p(desc), cap, C.byref(n),
                                           C.byref(m)))
        return kps[:n.value], desc[:n.value], m.value

    def matches(self, pair, cap=65536):
        out = [np.zeros(cap, np.int32) for _ in range(4)]
        nq = C.c_int(0)
        _check(_lib.orbgpu_download_matches(self.ctx.handle, pair, *[_p(o) for o in out], cap,
                                            C.byref(nq)))
        return tuple(o[:nq.value] for o in out)

    def stereo_matches(self, mbf, mb, stream=None):
        """Frame::ComputeStereoMatches (Frame.cc:827-997) for every pair 2p / 2p+1 of the last
        run(); results stay in HBM (stereo_result)."""
        _check(_lib.orbgpu_stereo_matches_batch(self.ctx.handle, self.n // 2, C.c_float(mbf),
                                                C.c_float(mb), C.c_void_p(stream) if stream else None))

    def stereo_result(self, pair, cap=65536):
        """(mvuRight, mvDepth, sad) of pair `pair`: float32, float32, int32 per left keypoint."""
        ur = np.zeros(cap, np.float32)
        dp = np.zeros(cap, np.float32)
        sad = np.zeros(cap, np.int32)
        n = C.c_int(0)
        _check(_lib.orbgpu_download_stereo(self.ctx.handle, pair, _p(ur), _p(dp), _p(sad), cap,
                                           C.byref(n)))
        return ur[:n.value], dp[:n.value], sad[:n.value]

    def fisheye_stereo(self, rig, stream=None):
        """Frame::ComputeStereoFishEyeMatches (Frame.cc:1142-1201) for every pair 2p / 2p+1 of the
        last run(): the stereo-row kNN2 (matches() returns it afterwards) and the KannalaBrandt8
        triangulation (rig: KB8Rig); results stay in HBM (fisheye_result)."""
        _check(_lib.orbgpu_fisheye_stereo_batch(self.ctx.handle, self.n // 2, C.byref(rig),
                                                C.c_void_p(stream) if stream else None))

    def fisheye_result(self, pair, cap=65536):
        """dict(l2r, r2l, depth, p3d, n_matches) of pair `pair` (mvLeftToRightMatch,
        mvRightToLeftMatch, mvDepth, mvStereo3Dpoints)."""
        l2r = np.zeros(cap, np.int32)
        r2l = np.zeros(cap, np.int32)
        dp = np.zeros(cap, np.float32)
        p3 = np.zeros((cap, 3), np.float32)
        nl, nr, nm = C.c_int(0), C.c_int(0), C.c_int(0)
        _check(_lib.orbgpu_download_fisheye(self.ctx.handle, pair, _p(l2r), _p(r2l), _p(dp), _p(p3), cap,
                                            C.byref(nl), C.byref(nr), C.byref(nm)))
        return dict(l2r=l2r[:nl.value], r2l=r2l[:nr.value], depth=dp[:nl.value], p3d=p3[:nl.value],
                    n_matches=nm.value)

    def upload_sbs(self, frames, width=None):
        """Side-by-side stereo Y8 frames [n, H, S] (row stride S >= 2W; W = S // 2 by default) ->
        images 2f (left half) and 2f + 1 (right half) of the batch (ORBextractor.cc:131-143)."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        n, h, stride = frames.shape
        w = stride // 2 if width is None else int(width)
        _check(_lib.orbgpu_upload_sbs(self.ctx.handle, _p(frames), n, w, h, stride))
        self.n, self.height, self.width = 2 * n, h, w
        self._staged = None

    def ingest_sbs(self, device_ptr, n_frames, stride, stream=None):
        """Split side-by-side frames already in device memory (zero-copy ingest)."""
        _check(_lib.orbgpu_ingest_sbs(self.ctx.handle, C.c_void_p(device_ptr), int(n_frames), self.width,
                                      self.height, int(stride), C.c_void_p(stream) if stream else None))
        self.n = 2 * int(n_frames)
        self._staged = None

    def pack_soa(self, n_pairs=None, stream=None):
        """The orbslam3.idl SoA layout for every image (and n_pairs stereo pairs' matches)."""
        npairs = self.n // 2 if n_pairs is None else int(n_pairs)
        _check(_lib.orbgpu_pack_soa(self.ctx.handle, self.n, npairs, C.c_void_p(stream) if stream else None))

    def soa_result(self, image, cap=65536):
        """dict(x, y, angle, level: int32 [n], orb: uint8 [n, 32], mono: int)."""
        a = {k: np.zeros(cap, np.int32) for k in ("x", "y", "angle", "level")}
        orb = np.zeros((cap, 32), np.uint8)
        n, m = C.c_int(0), C.c_int(0)
        _check(_lib.orbgpu_download_soa(self.ctx.handle, image, _p(a["x"]), _p(a["y"]), _p(a["angle"]),
                                        _p(a["level"]), _p(orb), cap, C.byref(n), C.byref(m)))
        out = {k: v[:n.value] for k, v in a.items()}
        out["orb"] = orb[:n.value]
        out["mono"] = m.value
        return out

    def matches16(self, pair, cap=65536):
        """(indices, distances1, distances2) int16 of stereo pair `pair` after pack_soa."""
        r = [np.zeros(cap, np.int16) for _ in range(3)]
        n = C.c_int(0)
        _check(_lib.orbgpu_download_matches16(self.ctx.handle, pair, _p(r[0]), _p(r[1]), _p(r[2]), cap,
                                              C.byref(n)))
        return tuple(a[:n.value] for a in r)

    @staticmethod
    def _map_point_rows(map_points, dtype=MAP_POINT_DTYPE, n=None):
        """(points, offsets, n_frames) for the C ABI: map_points is either a list (one per frame)
        of `dtype` arrays (MAP_POINT_DTYPE; LAST_POINT_DTYPE for track_by_projection), concatenated
        here, or a tuple (points, offsets) already in the ABI's form -- every frame's points in one
        array and int32 offsets [n + 1] -- which is passed through without a host copy.  n: the
        searches over pairs give their pair count; their offsets need only lie inside the points."""
        if isinstance(map_points, tuple):
            mps, off = map_points
            mps = np.ascontiguousarray(mps, dtype).reshape(-1)
            off = np.ascontiguousarray(off, np.int32)
            if n is None:
                if off.ndim != 1 or len(off) < 1 or off[0] != 0 or off[-1] != len(mps) or np.any(np.diff(off) < 0):
                    raise ValueError("map point offsets must start at 0, not decrease and end at len(points)")
            elif off.ndim != 1 or len(off) != n + 1 or off.min() < 0 or off.max() > len(mps):
                raise ValueError("keyframe offsets: one entry per pair plus one, inside the points")
            return mps, off, len(off) - 1
        if n is not None and len(map_points) != n:
            raise ValueError("one array of keyframe points per pair")
        rows = [np.asarray(m, dtype).reshape(-1) for m in map_points]
        mps = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros(0, dtype))
        off = np.zeros(len(rows) + 1, np.int32)
        off[1:] = np.cumsum([len(m) for m in rows])
        return mps, off, len(rows)

    @staticmethod
    def _pad_rows(rows, dtype, fill, n=None, inner=()):
        """(array [n, stride, *inner], stride) of `fill`-padded rows for the C ABI, (None, 0) for None:
        rows is a list of 1-D (inner == (2,): [k, 2]) rows, n of them (None: len(rows)), or one array
        that is padded already, which is passed through."""
        if rows is None:
            return None, 0
        if isinstance(rows, np.ndarray) and rows.ndim == 2 + len(inner) and (
                n is None or (rows.shape[0] == n and rows.shape[1] > 0)):
            out = np.ascontiguousarray(rows, dtype)
        else:
            rows = [np.asarray(r, dtype).reshape((-1,) + inner) for r in rows]
            out = np.full((len(rows) if n is None else n, max([1] + [len(r) for r in rows])) + inner, fill, dtype)
            for p, r in enumerate(rows):
                out[p, :len(r)] = r
        return out, out.shape[1]

    def _download_matches(self, fn, row, cap):
        """(match [n_kp] int32, nmatches, rot_hist [30] int32) of result row `row` through fn."""
        m = np.zeros(cap, np.int32)
        h = np.zeros(30, np.int32)
        n, nm = C.c_int(0), C.c_int(0)
        _check(fn(self.ctx.handle, row, _p(m), cap, C.byref(n), C.byref(nm), _p(h)))
        return m[:n.value], nm.value, h

    def search_by_projection(self, map_points, image_step=2, use_uright=True, kp_block=None, th=1.0,
                             nnratio=0.8, far_points=False, th_far=50.0, stream=None):
        """ORBmatcher(nnratio).SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints)
        (ORBmatcher.cc:44-214) for frames f = images f * image_step after undistort_grid();
        map_points: list (one per frame) of MAP_POINT_DTYPE arrays, or (points, offsets) with every
        frame's points in one array (_map_point_rows); kp_block: optional list of u8 arrays (1 =
        keypoint already holds a map point with observations)."""
        mps, off, nf = self._map_point_rows(map_points)
        blk, stride = self._pad_rows(kp_block, np.uint8, 0, nf)
        _check(_lib.orbgpu_search_by_projection_batch(
            self.ctx.handle, nf, int(image_step), int(use_uright), _p(mps) if len(mps) else None, _p(off),
            _p(blk) if blk is not None else None, stride, C.c_float(th), C.c_float(nnratio),
            int(far_points), C.c_float(th_far), C.c_void_p(stream) if stream else None))

    def search_by_projection_stereo(self, map_points, left_to_right=None, right_to_left=None, kp_block=None,
                                    th=1.0, nnratio=0.8, far_points=False, th_far=50.0, stream=None):
        """The two-camera SearchByProjection (Nleft != -1, ORBmatcher.cc:59-214) on every stereo
        pair of the last run() (grids from undistort_grid(K, ())); left_to_right / right_to_left:
        per pair int32 arrays (mvLeftToRightMatch / mvRightToLeftMatch); kp_block per pair over
        Nleft + Nright keypoints; map_points as for search_by_projection."""
        mps, off, nf = self._map_point_rows(map_points)
        l2r, lrs = self._pad_rows(left_to_right, np.int32, -1, nf)
        r2l, lrs2 = self._pad_rows(right_to_left, np.int32, -1, nf)
        if l2r is not None and r2l is not None and lrs != lrs2:
            w = max(lrs, lrs2)
            l2r = np.pad(l2r, ((0, 0), (0, w - lrs)), constant_values=-1)
            r2l = np.pad(r2l, ((0, 0), (0, w - lrs2)), constant_values=-1)
            lrs = w
        lrs = lrs or lrs2
        blk, bst = self._pad_rows(kp_block, np.uint8, 0, nf)
        _check(_lib.orbgpu_search_by_projection_stereo(
            self.ctx.handle, nf, _p(mps) if len(mps) else None, _p(off),
            _p(l2r) if l2r is not None else None, _p(r2l) if r2l is not None else None, lrs,
            _p(blk) if blk is not None else None, bst, C.c_float(th), C.c_float(nnratio), int(far_points),
            C.c_float(th_far), C.c_void_p(stream) if stream else None))

    def projection_matches(self, frame, cap=65536):
        """(match [n_kp] int32: map point index or -1, nmatches) of frame `frame`."""
        m = np.zeros(cap, np.int32)
        n, nm = C.c_int(0), C.c_int(0)
        _check(_lib.orbgpu_download_projection_matches(self.ctx.handle, frame, _p(m), cap, C.byref(n),
                                                       C.byref(nm)))
        return m[:n.value], nm.value

    def track_by_projection(self, points, poses, K, mbf, mb, image_step=2, use_uright=True, kp_block=None,
                            th=15.0, mono=False, check_orientation=True, stream=None):
        """ORBmatcher(nnratio, check_orientation).SearchByProjection(CurrentFrame, LastFrame, th, mono)
        (ORBmatcher.cc:1683-1838, Tracking::TrackWithMotionModel) for frames f = images f * image_step
        after undistort_grid(); points: list (one per frame) of LAST_POINT_DTYPE arrays, or (points,
        offsets) as for search_by_projection; poses: TRACK_POSE_DTYPE array, one row per frame;
        K = (fx, fy, cx, cy); kp_block as for search_by_projection."""
        pts, off, nf = self._map_point_rows(points, LAST_POINT_DTYPE)
        ps = np.ascontiguousarray(poses, TRACK_POSE_DTYPE).reshape(-1)
        if len(ps) != nf:
            raise ValueError("one pose per frame")
        Kf = np.ascontiguousarray(K, dtype=np.float32).reshape(4)
        blk, stride = self._pad_rows(kp_block, np.uint8, 0, nf)
        _check(_lib.orbgpu_track_by_projection_batch(
            self.ctx.handle, nf, int(image_step), int(use_uright), _p(pts) if len(pts) else None, _p(off), _p(ps),
            _p(Kf), C.c_float(mbf), C.c_float(mb), _p(blk) if blk is not None else None, stride, C.c_float(th),
            int(mono), int(check_orientation), C.c_void_p(stream) if stream else None))

    def track_by_projection_stereo(self, points, poses, rig, mb, kp_block=None, th=15.0, mono=False,
                                   check_orientation=True, stream=None):
        """The two-camera form (CurrentFrame.Nleft != -1, ORBmatcher.cc:1721-1921 with :1840-1914)
        on every stereo pair of the last run() (grids from undistort_grid(K, ())); points and poses
        as for track_by_projection, the points covering the last frame's Nleft + Nright keypoints;
        rig: a TRACK_RIG_DTYPE record (cam_left, Rrl, trl); kp_block per pair over Nleft + Nright
        keypoints.  track_matches(frame) then covers Nleft + Nright keypoints, left first."""
        pts, off, nf = self._map_point_rows(points, LAST_POINT_DTYPE)
        ps = np.ascontiguousarray(poses, TRACK_POSE_DTYPE).reshape(-1)
        if len(ps) != nf:
            raise ValueError("one pose per frame")
        rg = None
        if rig is not None:
            rg = np.ascontiguousarray(rig, TRACK_RIG_DTYPE).reshape(-1)
            if len(rg) != 1:
                raise ValueError("one rig")
        blk, stride = self._pad_rows(kp_block, np.uint8, 0, nf)
        _check(_lib.orbgpu_track_by_projection_stereo(
            self.ctx.handle, nf, _p(pts) if len(pts) else None, _p(off), _p(ps), _p(rg) if rg is not None else None,
            C.c_float(mb), _p(blk) if blk is not None else None, stride, C.c_float(th), int(mono),
            int(check_orientation), C.c_void_p(stream) if stream else None))

    def track_matches(self, frame, cap=65536):
        """(match [n_kp] int32: last-frame point index or -1, nmatches, rot_hist [30] int32: the bin
        sizes before the three-maxima rule) of frame `frame`; n_kp = Nleft + Nright after
        track_by_projection_stereo."""
        return self._download_matches(_lib.orbgpu_download_track_matches, frame, cap)

    def search_for_initialization(self, image_pairs, prev_matched=None, window_size=100, nnratio=0.9,
                                  check_orientation=True, stream=None):
        """ORBmatcher(nnratio, check_orientation).SearchForInitialization(F1, F2, vbPrevMatched,
        vnMatches12, windowSize) (ORBmatcher.cc:649-764, Tracking::MonocularInitialization) for pairs
        (F1, F2) of batch images after undistort_grid(); prev_matched: a list (one per pair) of
        [n1, 2] float32 arrays, or one padded [n_pairs, stride, 2] array; None: F1's mvKeysUn.pt."""
        pairs = np.ascontiguousarray(image_pairs, np.int32).reshape(-1, 2)
        pm, stride = self._pad_rows(prev_matched, np.float32, 0, inner=(2,))
        if pm is not None and (pm.shape[0] != len(pairs) or pm.shape[2] != 2):
            raise ValueError("one row of [n1, 2] points per pair")
        _check(_lib.orbgpu_search_for_initialization_batch(
            self.ctx.handle, len(pairs), _p(pairs) if len(pairs) else None, _p(pm) if pm is not None else None,
            stride, int(window_size), C.c_float(nnratio), int(check_orientation),
            C.c_void_p(stream) if stream else None))

    def initialization_matches(self, pair, cap=65536):
        """(match12 [n1] int32: vnMatches12, prev_matched [n1, 2] float32: vbPrevMatched after the
        call, nmatches, rot_hist [30] int32: the bin sizes before the three-maxima rule) of pair
        `pair` of the last search_for_initialization."""
        m = np.zeros(cap, np.int32)
        pm = np.zeros((cap, 2), np.float32)
        h = np.zeros(30, np.int32)
        n, nm = C.c_int(0), C.c_int(0)
        _check(_lib.orbgpu_download_initialization_matches(self.ctx.handle, pair, _p(m), _p(pm), cap, C.byref(n),
                                                           C.byref(nm), _p(h)))
        return m[:n.value], pm[:n.value], nm.value, h

    def search_by_bow(self, frames, kf_points, f_nodes, nnratio=0.7, check_orientation=True, stream=None):
        """ORBmatcher(nnratio, check_orientation).SearchByBoW(pKF, F, vpMapPointMatches) (ORBmatcher.cc:
        224-426, Tracking::TrackReferenceKeyFrame / Relocalization; pinhole frames) for pairs of a
        keyframe and a batch image of the last run(); undistort_grid() is not needed.  frames: the
        batch image of each pair (one image may serve several pairs); kf_points: a list (one per
        pair) of BOW_POINT_DTYPE arrays, or (points, offsets) in the C ABI's form; f_nodes: a list of
        int32 arrays (the node of each keypoint of the pair's frame, < 0: none) or one 2-D array
        [n_pairs, stride]."""
        fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
        npairs = len(fr)
        pts, off, _ = self._map_point_rows(kf_points, BOW_POINT_DTYPE, npairs)
        nodes, _ = self._pad_rows(f_nodes, np.int32, -1)
        if nodes.shape[0] != npairs:
            raise ValueError("one row of nodes per pair")
        _check(_lib.orbgpu_search_by_bow_batch(
            self.ctx.handle, npairs, _p(fr) if npairs else None, _p(pts) if npairs else None,
            _p(off) if npairs else None, _p(nodes) if npairs else None, nodes.shape[1] if npairs else 0,
            C.c_float(nnratio), int(check_orientation), C.c_void_p(stream) if stream else None))

    def bow_matches(self, pair, cap=65536):
        """(match [N] int32: for each keypoint of F the index, within the pair's keyframe points, of
        the point that ends up in vpMapPointMatches, -1 if none; nmatches; rot_hist [30] int32: the
        bin sizes before the three-maxima rule) of pair `pair` of the last search_by_bow."""
        return self._download_matches(_lib.orbgpu_download_bow_matches, pair, cap)

    def search_for_triangulation(self, frames, kf_points, pairs, f_nodes, f_flags=None, only_stereo=False,
                                 coarse=False, check_orientation=False, stream=None):
        """ORBmatcher(nnratio, check_orientation).SearchForTriangulation(pKF1, pKF2, vMatchedPairs,
        bOnlyStereo, bCoarse) (ORBmatcher.cc:908-1153, LocalMapping::CreateNewMapPoints; pinhole
        keyframes) for pairs of a batch image after undistort_grid() (keyframe 1) and a keyframe the
        host gives (keyframe 2).  frames: the batch image of each pair (one image may serve several
        pairs); kf_points: a list (one per pair) of TRIANG_POINT_DTYPE arrays, or (points, offsets)
        in the C ABI's form; pairs: TRIANG_PAIR_DTYPE array, one row per pair (F12 and the epipole);
        f_nodes: a list of int32 arrays (the node of each keypoint of keyframe 1, < 0: none) or one
        2-D array [n_pairs, stride]; f_flags: the same shape in uint8 with TRI_HAS_POINT /
        TRI_STEREO per keypoint of keyframe 1, None: neither anywhere."""
        fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
        npairs = len(fr)
        pts, off, _ = self._map_point_rows(kf_points, TRIANG_POINT_DTYPE, npairs)
        pr = np.ascontiguousarray(pairs, TRIANG_PAIR_DTYPE).reshape(-1)
        if len(pr) != npairs:
            raise ValueError("one F12 and epipole per pair")
        nodes, _ = self._pad_rows(f_nodes, np.int32, -1)
        if nodes.shape[0] != npairs:
            raise ValueError("one row of nodes per pair")
        flg, fstride = self._pad_rows(f_flags, np.uint8, 0)
        if flg is not None and flg.shape[0] != npairs:
            raise ValueError("one row of flags per pair")
        _check(_lib.orbgpu_search_for_triangulation_batch(
            self.ctx.handle, npairs, _p(fr) if npairs else None, _p(pts) if npairs else None,
            _p(off) if npairs else None, _p(pr) if npairs else None, _p(nodes) if npairs else None,
            nodes.shape[1] if npairs else 0, _p(flg) if flg is not None and npairs else None, fstride,
            int(only_stereo), int(coarse), int(check_orientation), C.c_void_p(stream) if stream else None))

    def triangulation_matches(self, pair, cap=65536):
        """(match12 [N1] int32: for each keypoint of keyframe 1 the index, within the pair's keyframe
        points, left in vMatches12, -1 if none; nmatches; rot_hist [30] int32: the bin sizes before the
        three-maxima rule) of pair `pair` of the last search_for_triangulation.  vMatchedPairs =
        [(k, match12[k]) for k in np.flatnonzero(match12 >= 0)]."""
        return self._download_matches(_lib.orbgpu_download_triangulation_matches, pair, cap)

    def search_by_bow_kf(self, frames, kf_points, f_nodes, f_flags=None, nnratio=0.9, check_orientation=True,
                         stream=None):
        """ORBmatcher(nnratio, check_orientation).SearchByBoW(pKF1, pKF2, vpMatches12) (ORBmatcher.cc:766-906,
        LoopClosing::DetectCommonRegionsFromBoW; pinhole keyframes) for pairs of a batch image of the last
        run() (keyframe 1; undistort_grid() is not needed) and a keyframe the host gives (keyframe 2).  The
        defaults are that caller's matcher, ORBmatcher matcherBoW(0.9, true) (LoopClosing.cc:591).  frames:
        the batch image of each pair (one current keyframe usually serves all 6 to 18 pairs of a call);
        kf_points: a list (one per pair) of BOWKF_POINT_DTYPE arrays, or (points, offsets) in the C ABI's
        form; f_nodes: a list of int32 arrays (the node of each keypoint of keyframe 1, < 0: none) or one
        2-D array [n_pairs, stride]; f_flags: the same shape in uint8 with BOWKF_HAS_POINT per keypoint of
        keyframe 1, None: every keypoint has a map point."""
        fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
        npairs = len(fr)
        pts, off, _ = self._map_point_rows(kf_points, BOWKF_POINT_DTYPE, npairs)
        nodes, _ = self._pad_rows(f_nodes, np.int32, -1)
        if nodes.shape[0] != npairs:
            raise ValueError("one row of nodes per pair")
        flg, fstride = self._pad_rows(f_flags, np.uint8, 0)
        if flg is not None and flg.shape[0] != npairs:
            raise ValueError("one row of flags per pair")
        _check(_lib.orbgpu_search_by_bow_kf_batch(
            self.ctx.handle, npairs, _p(fr) if npairs else None, _p(pts) if npairs else None,
            _p(off) if npairs else None, _p(nodes) if npairs else None, nodes.shape[1] if npairs else 0,
            _p(flg) if flg is not None and npairs else None, fstride, C.c_float(nnratio), int(check_orientation),
            C.c_void_p(stream) if stream else None))

    def bow_kf_matches(self, pair, cap=65536):
        """(match12 [N1] int32: for each keypoint of keyframe 1 the index, within the pair's keyframe points,
        left in vpMatches12, -1 if none; nmatches; rot_hist [30] int32: the bin sizes before the
        three-maxima rule; code [N1] uint8: BOWKF_*; best [N1, 2] int16: bestDist1, bestDist2 of the
        keypoint's walk, 256 where a side found nothing, 0 where there was no walk) of pair `pair` of the
        last search_by_bow_kf.  vpMatches12[k] = vpMapPoints2[match12[k]]."""
        m = np.zeros(cap, np.int32)
        code = np.zeros(cap, np.uint8)
        best = np.zeros((cap, 2), np.int16)
        h = np.zeros(30, np.int32)
        n, nm = C.c_int(0), C.c_int(0)
        _check(_lib.orbgpu_download_bow_kf_matches(self.ctx.handle, pair, _p(m), _p(code), _p(best), cap, C.byref(n),
                                                   C.byref(nm), _p(h)))
        return m[:n.value], nm.value, h, code[:n.value], best[:n.value]

    def reloc_by_projection(self, frames, kf_points, poses, K, kp_block=None, th=10.0, orb_dist=100,
                            check_orientation=True, stream=None):
        """ORBmatcher(0.9, check_orientation).SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th,
        ORBdist) (ORBmatcher.cc:1923-2059, Tracking::Relocalization; pinhole frames) for pairs of a
        keyframe's map points and a batch image after undistort_grid().  frames: the batch image of
        each pair (one image may serve several pairs); kf_points: a list (one per pair) of
        RELOC_POINT_DTYPE arrays, or (points, offsets) in the C ABI's form; poses: RELOC_POSE_DTYPE
        array, one row per pair; K = (fx, fy, cx, cy); kp_block: optional list (one per pair) of u8
        arrays, or one 2-D array (non-zero = the keypoint already holds a map point)."""
        fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
        npairs = len(fr)
        pts, off, _ = self._map_point_rows(kf_points, RELOC_POINT_DTYPE, npairs)
        ps = np.ascontiguousarray(poses, RELOC_POSE_DTYPE).reshape(-1)
        if len(ps) != npairs:
            raise ValueError("one pose per pair")
        Kf = np.ascontiguousarray(K, dtype=np.float32).reshape(4)
        blk, stride = self._pad_rows(kp_block, np.uint8, 0)
        if blk is not None and blk.shape[0] != npairs:
            raise ValueError("one row of occupancy per pair")
        _check(_lib.orbgpu_reloc_by_projection_batch(
            self.ctx.handle, npairs, _p(fr) if npairs else None, _p(pts) if len(pts) else None,
            _p(off) if npairs else None, _p(ps) if npairs else None, _p(Kf),
            _p(blk) if blk is not None and npairs else None, stride, C.c_float(th), int(orb_dist),
            int(check_orientation), C.c_void_p(stream) if stream else None))

    def reloc_matches(self, pair, cap=65536):
        """(match [N] int32: for each keypoint of the frame the index, within the pair's keyframe
        points, of the point this call put into mvpMapPoints, -1 if none; nmatches; rot_hist [30]
        int32: the bin sizes before the three-maxima rule) of pair `pair` of the last
        reloc_by_projection."""
        return self._download_matches(_lib.orbgpu_download_reloc_matches, pair, cap)

    def fuse(self, frames, lists, point_lists, poses, K, skip=None, th=3.0, bf=0.0, use_uright=False, sim3=False,
             stream=None):
        """ORBmatcher::Fuse(pKF, vpMapPoints, th) (ORBmatcher.cc:1155-1345, LocalMapping::SearchInNeighbors;
        pinhole keyframes) and, with sim3, the Sim3 overload (:1347-1462, LoopClosing::SearchAndFuse) for
        pairs of a list of map points and a batch image after undistort_grid().  frames: the batch image
        of each pair; lists: the list each pair fuses (several pairs may name one list, or one frame);
        point_lists: a list of FUSE_POINT_DTYPE arrays, or (points, offsets) in the C ABI's form;
        poses: RELOC_POSE_DTYPE array, one row per pair (Rcw, tcw, Ow); K = (fx, fy, cx, cy); skip:
        optional list (one per pair) of u8 arrays over the pair's list, or one 2-D array (non-zero = the
        point is already in that keyframe); bf = pKF->mbf; use_uright: the keypoints with a right
        coordinate (after stereo_matches; every frame a left image) take the stereo chi-square gate."""
        fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
        ls = np.ascontiguousarray(lists, np.int32).reshape(-1)
        npairs = len(fr)
        if len(ls) != npairs:
            raise ValueError("one list index per pair")
        if isinstance(point_lists, tuple):
            pts, off, nl = self._map_point_rows(point_lists, FUSE_POINT_DTYPE, len(point_lists[1]) - 1)
        else:
            pts, off, nl = self._map_point_rows(point_lists, FUSE_POINT_DTYPE)
        ps = np.ascontiguousarray(poses, RELOC_POSE_DTYPE).reshape(-1)
        if len(ps) != npairs:
            raise ValueError("one pose per pair")
        Kf = np.ascontiguousarray(K, dtype=np.float32).reshape(4)
        sk, stride = self._pad_rows(skip, np.uint8, 0)
        if sk is not None and sk.shape[0] != npairs:
            raise ValueError("one row of skip flags per pair")
        _check(_lib.orbgpu_fuse_batch(
            self.ctx.handle, npairs, _p(fr) if npairs else None, _p(ls) if npairs else None, nl,
            _p(pts) if len(pts) else None, _p(off), _p(ps) if npairs else None, _p(Kf),
            _p(sk) if sk is not None and npairs else None, stride, C.c_float(th), C.c_float(bf), int(use_uright),
            int(sim3), C.c_void_p(stream) if stream else None))

    def fuse_matches(self, pair, cap_points=FUSE_MAX_POINTS, cap_kp=65536):
        """(best_idx [n] int32: the keypoint point i fused onto, else -1; best_dist [n] int32: the lowest
        distance that survived the filters, 256 if none; code [n] uint8: FUSE_*; first [N] int32: for
        each keypoint of the frame the lowest point that fused onto it, -1 if none; nfused) of pair
        `pair` of the last fuse."""
        bi = np.zeros(cap_points, np.int32)
        bd = np.zeros(cap_points, np.int32)
        cd = np.zeros(cap_points, np.uint8)
        first = np.zeros(cap_kp, np.int32)
        n, nk, nf = C.c_int(0), C.c_int(0), C.c_int(0)
        _check(_lib.orbgpu_download_fuse_matches(self.ctx.handle, pair, _p(bi), _p(bd), _p(cd), cap_points, _p(first),
                                                 cap_kp, C.byref(n), C.byref(nk), C.byref(nf)))
        return bi[:n.value], bd[:n.value], cd[:n.value], first[:nk.value], nf.value

    def sim3_search_by_projection(self, frames, lists, point_lists, poses, K, skip=None, kp_block=None, th=8.0,
                                  ratio_hamming=1.5, projection=SIM3_PROJECT_DIV, stream=None):
        """ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) (ORBmatcher.cc:
        428-533; projection = SIM3_PROJECT_DIV) and the overload with vpPointsKFs / vpMatchedKF (:535-647;
        SIM3_PROJECT_INVZ), LoopClosing::DetectCommonRegionsFromBoW / FindMatchesByProjection; pinhole
        keyframes, for pairs of a list of map points and a batch image after undistort_grid().  frames,
        lists, point_lists (FUSE_POINT_DTYPE), poses (RELOC_POSE_DTYPE rows from Scw: Rcw, tcw / s, Ow), K
        and skip (spAlreadyFound) as for fuse; kp_block: optional list (one per pair) of u8 arrays, or one
        2-D array (non-zero = vpMatched[k] is set before the call).  Each pair is one call of the
        reference with its own vpMatched."""
        fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
        ls = np.ascontiguousarray(lists, np.int32).reshape(-1)
        npairs = len(fr)
        if len(ls) != npairs:
            raise ValueError("one list index per pair")
        if isinstance(point_lists, tuple):
            pts, off, nl = self._map_point_rows(point_lists, FUSE_POINT_DTYPE, len(point_lists[1]) - 1)
        else:
            pts, off, nl = self._map_point_rows(point_lists, FUSE_POINT_DTYPE)
        ps = np.ascontiguousarray(poses, RELOC_POSE_DTYPE).reshape(-1)
        if len(ps) != npairs:
            raise ValueError("one pose per pair")
        Kf = np.ascontiguousarray(K, dtype=np.float32).reshape(4)
        sk, stride = self._pad_rows(skip, np.uint8, 0)
        if sk is not None and sk.shape[0] != npairs:
            raise ValueError("one row of skip flags per pair")
        blk, kstride = self._pad_rows(kp_block, np.uint8, 0)
        if blk is not None and blk.shape[0] != npairs:
            raise ValueError("one row of occupancy per pair")
        _check(_lib.orbgpu_sim3_search_by_projection_batch(
            self.ctx.handle, npairs, _p(fr) if npairs else None, _p(ls) if npairs else None, nl,
            _p(pts) if len(pts) else None, _p(off), _p(ps) if npairs else None, _p(Kf),
            _p(sk) if sk is not None and npairs else None, stride, _p(blk) if blk is not None and npairs else None,
            kstride, C.c_float(th), C.c_float(ratio_hamming), int(projection), C.c_void_p(stream) if stream else None))

    def sim3_matches(self, pair, cap_points=FUSE_MAX_POINTS, cap_kp=65536):
        """(match [N] int32: for each keypoint of the frame the list index of the point this call put on
        it, -1 if none (vpMatchedKF[k] = vpPointsKFs[match[k]]); best_idx [n] int32: the keypoint point i
        matched, else -1; best_dist [n] int32: its distance when matched, else 256; code [n] uint8:
        SIM3_*; nmatches) of pair `pair` of the last sim3_search_by_projection."""
        m = np.zeros(cap_kp, np.int32)
        bi = np.zeros(cap_points, np.int32)
        bd = np.zeros(cap_points, np.int32)
        cd = np.zeros(cap_points, np.uint8)
        nk, n, nm = C.c_int(0), C.c_int(0), C.c_int(0)
        _check(_lib.orbgpu_download_sim3_matches(self.ctx.handle, pair, _p(m), cap_kp, _p(bi), _p(bd), _p(cd), cap_points,
                                                 C.byref(nk), C.byref(n), C.byref(nm)))
        return m[:nk.value], bi[:n.value], bd[:n.value], cd[:n.value], nm.value

    def sim3_replay_stats(self, pair):
        """(points that reached the replay, passes, lanes found stale over all passes, windows walked
        again) of pair `pair` of the last sim3_search_by_projection: what tools/sim3_search_time.py prints."""
        s = np.zeros(4, np.int32)
        _check(_lib.orbgpu_sim3_replay_stats(self.ctx.handle, pair, _p(s)))
        return tuple(int(v) for v in s)

    def undistort_grid(self, K, dist=(), stream=None):
        """Frame::UndistortKeyPoints + AssignFeaturesToGrid (Frame.cc:405-436, 741-825) for every
        image of the last run(); K = (fx, fy, cx, cy), dist = (k1, k2, p1, p2[, k3])."""
        Kf = np.ascontiguousarray(K, dtype=np.float32)
        d = np.ascontiguousarray(dist, dtype=np.float32)
        _check(_lib.orbgpu_undistort_grid_batch(self.ctx.handle, self.n, _p(Kf), _p(d) if len(d) else None,
                                                len(d), C.c_void_p(stream) if stream else None))

    def grid_result(self, image, cap=65536):
        """(xy_un [n,2], cell [n], cell_start [3073], cell_idx) of image `image`."""
        xy = np.zeros((cap, 2), np.float32)
        cell = np.zeros(cap, np.int32)
        cs = np.zeros(64 * 48 + 1, np.int32)
        ci = np.zeros(cap, np.int32)
        n = C.c_int(0)
        _check(_lib.orbgpu_download_grid(self.ctx.handle, image, _p(xy), _p(cell), _p(cs), _p(ci), cap,
                                         C.byref(n)))
        return xy[:n.value], cell[:n.value], cs, ci[:cs[-1]]

    def set_profiling(self, on=True, stages=None, serialize=False):
        """on: bracket every stage's launches with HIP events; stages: only these stage names;
        serialize: launch each stage once over the whole batch (clean per-kernel durations)."""
        names = [_lib.orbgpu_stage_name(i).decode() for i in range(_lib.orbgpu_num_stages())]
        if not on:
            arg = C.c_int(0)
        elif stages is None and not serialize:
            arg = C.c_int(1)
        else:
            mask = 0
            for st in (names if stages is None else stages):
                mask |= 1 << names.index(st)
            word = (1 << 31) | (1 << 30 if serialize else 0) | mask
            arg = C.c_int(word - (1 << 32))  # the flag word as a signed int
        _check(_lib.orbgpu_set_profiling(self.ctx.handle, arg))

    def reset_stage_times(self):
        _check(_lib.orbgpu_reset_stage_times(self.ctx.handle))

    def stage_times(self):
        ns = _lib.orbgpu_num_stages()
        ms = np.zeros(ns, np.float64)
        cnt = np.zeros(ns, np.int64)
        _check(_lib.orbgpu_stage_times(self.ctx.handle, _p(ms), _p(cnt), ns))
        return {_lib.orbgpu_stage_name(i).decode(): (float(ms[i]), int(cnt[i])) for i in range(ns)}
