"""TEST INFRASTRUCTURE ONLY (host side of tests/test_gpu_stale_memory.py): the memory-poisoning replacement of torch's
uninitialised allocators, bit-exact comparison (`snapshot`, `differences`: the one copy every family imports), the parser that lists
every entry point of the public headers (rohm_amd._lib.HEADERS, read together) taking a caller-owned buffer, and the coverage list
that names the case(s) exercising each of them; for tests/test_gpu_bounds.py also the parser that lists every entry point with a
pointer to numbers (`abi_pointer_functions`) and its exemptions.

include/rohm_hip.h ("Caller-owned memory") promises that `ws`, `scratch`, `saved` and output buffers may hold anything on
entry.  Every Python wrapper gets them from torch.empty / empty_like / new_empty; `poison` replaces those three for the
duration of a test by versions that fill what they return with a byte pattern, so a kernel that reads a word it did not
write computes with that pattern instead of the zeros of a fresh process."""
import contextlib
import os
import re

import torch

# 32-bit words, little-endian bytes.  Each shows a bug one of the others hides:
#   ones    0xFFFFFFFF  fp32 / fp64 NaN, int -1, uint max: survives 0 * x (pad columns that rely on zero weights); leaves an
#                       exchange header un-armed with every slot "tagged"
#   small   0x01010101  a denormal-sized float, a small positive int, a uint that WINS an atomicMin (all-ones is the "far"
#                       value of the z-buffers and would hide an unset depth cell)
#   fltmax  0x7F7FFFFF  FLT_MAX: finite, so it passes through fmaxf / fminf / comparisons that drop NaN; any sum overflows
PATTERNS = {'ones': b'\xff\xff\xff\xff', 'small': b'\x01\x01\x01\x01', 'fltmax': b'\xff\xff\x7f\x7f'}
ZEROS = b'\x00\x00\x00\x00'
_REAL_EMPTY = torch.empty      # (the un-patched allocator, for this module's own temporaries)


def fill_bytes(t, word):
    """Fill the whole storage behind `t` with the 4-byte pattern `word` (repeated from the storage's first byte)."""
    n = t.untyped_storage().nbytes()
    if n == 0:
        return t
    raw = _REAL_EMPTY(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())
    if len(set(word)) == 1:
        raw.fill_(word[0])
    else:
        raw.copy_(torch.tensor(list(word), dtype=torch.uint8, device=t.device).repeat((n + 3) // 4)[:n])
    return t


def install(monkeypatch, word, device_types=('cuda',)):
    """Replace torch.empty, torch.empty_like and Tensor.new_empty until `monkeypatch` is undone: same allocation, then
    tensors on a device type in `device_types` are filled with `word`.  torch.zeros and friends are left alone."""
    real_empty, real_like, real_new = torch.empty, torch.empty_like, torch.Tensor.new_empty

    def filled(t):
        return fill_bytes(t, word) if t.device.type in device_types else t

    def empty(*a, **k):
        return filled(real_empty(*a, **k))

    def empty_like(*a, **k):
        return filled(real_like(*a, **k))

    def new_empty(self, *a, **k):
        return filled(real_new(self, *a, **k))

    monkeypatch.setattr(torch, 'empty', empty)
    monkeypatch.setattr(torch, 'empty_like', empty_like)
    monkeypatch.setattr(torch.Tensor, 'new_empty', new_empty)


@contextlib.contextmanager
def poison(word, device_types=('cuda',)):
    """`install` as a context manager (its own MonkeyPatch, undone on exit)."""
    import pytest
    with pytest.MonkeyPatch.context() as m:
        install(m, word, device_types)
        yield


@contextlib.contextmanager
def env(**values):
    """Environment variables for the duration of a case (None removes one)."""
    old = {k: os.environ.get(k) for k in values}
    try:
        for k, v in values.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def bits(t):
    """The bytes of a tensor as a flat uint8 tensor on the CPU: NaN compares equal to the same NaN."""
    t = t.detach().contiguous().reshape(-1)
    return (t.view(torch.uint8) if t.numel() else _REAL_EMPTY(0, dtype=torch.uint8)).cpu()


def first_difference(a, b):
    """None if the two tensors are bit-identical, else (flat element index, value in a, value in b)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return ('shape/dtype', (tuple(a.shape), a.dtype), (tuple(b.shape), b.dtype))
    ba, bb = bits(a), bits(b)
    if torch.equal(ba, bb):
        return None
    i = int((ba != bb).nonzero()[0]) // a.element_size()
    fa, fb = a.detach().contiguous().reshape(-1), b.detach().contiguous().reshape(-1)
    return (i, fa[i].item(), fb[i].item())


# ---- the ABI's caller-owned buffers ------------------------------------------------------------------------------------------
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include')
_HEADERS = {}


def abi_headers():
    """{file name: text} of every public header, in the order of rohm_amd._lib.HEADERS (read once)."""
    if not _HEADERS:
        from rohm_amd import _lib
        for name in _lib.HEADERS:
            with open(os.path.join(INCLUDE, name)) as f:
                _HEADERS[name] = f.read()
    return dict(_HEADERS)


def abi_text():
    return '\n'.join(abi_headers().values())


def declarations(text=None):
    """[(entry point, [the text of each parameter])] of every `rohm_*(...);` declaration outside a comment, in order; `text`
    defaults to all public headers together."""
    text = re.sub(r'/\*.*?\*/', ' ', abi_text() if text is None else text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    return [(m.group(1), [p for p in m.group(2).split(',') if p.strip() not in ('', 'void')])
            for m in re.finditer(r'\b(rohm_\w+)\s*\(([^;{}()]*)\)\s*;', text)]


def abi_buffer_functions(text=None):
    """{entry point: [buffer names]} for every declaration with a `void* <name>, size_t <name>_bytes` (or `size_t bytes`) parameter
    pair (const or not): the functions that are handed a caller-owned workspace."""
    out = {}
    for name, params in declarations(text):
        names = [p.group(1) for p in re.finditer(r'void\s*\*\s*(\w+)\s*,\s*size_t\s+(\w*?)_?bytes\b', ','.join(params))
                 if p.group(2) in (p.group(1), '')]
        if names:
            out[name] = names
    return out


_POINTEE = r'(?:float|double|void|int|unsigned(?:\s+(?:char|int))?|long\s+long|size_t|u?int(?:8|16|32|64)_t)'


def abi_pointer_functions(text=None):
    """{entry point: [parameter names]} for every declaration with a parameter that points at numbers -- `float*`, `double*`,
    `void*`, an integer pointer, a table of such pointers (`float* const*`), const or not: every function that can be handed a
    caller's tensor.  Pointers to structs, handles and strings are not listed.  The headers do not say in their types which of these
    live on the host (plans, limits, camera matrices): POINTER_EXEMPT names the host-only calls one by one, and
    tests/test_guarded_memory_host.py holds every other function to a guarded-memory case."""
    out = {}
    for name, params in declarations(text):
        names = []
        for param in params:
            p = re.match(r'^\s*(?:const\s+)?' + _POINTEE + r'\s*(?:const\s*)?\*\s*(?:const\s*\*\s*)?(?:const\s+)?(\w+)\s*$', param)
            if p:
                names.append(p.group(1))
        if names:
            out[name] = names
    return out


# ---- one snapshot, one comparison ----------------------------------------------------------------------------------------------
def snapshot(out):
    """Clones of the tensors of [(label, tensor)], queued on the current stream (no wait)."""
    return [(label, t.detach().clone()) for label, t in out]


def differences(got, want):
    """[(label, first_difference)] of the outputs that are not bit-identical; the two lists must carry the same labels."""
    assert [l for l, _ in got] == [l for l, _ in want], ([l for l, _ in got], [l for l, _ in want])
    return [(label, d) for (label, a), (_, b) in zip(got, want) for d in [first_difference(a, b)] if d is not None]


# entry points with a pointer parameter that no guarded-memory case runs (tests/test_gpu_bounds.py), each with its reason
POINTER_EXEMPT = {
    'rohm_profile_stop': 'host-only: the row count goes to a host int, nothing on the device is touched',
    'rohm_output_process_plan': 'host-only: the launch plan is returned through two host ints',
    'rohm_adamw_limits': 'host-only: two host ints',
    'rohm_mv_limits': 'host-only: two host ints',
    'rohm_smplx_create': 'create: copies the model arrays into device memory the handle owns, sized by V, J and n_shape_total',
    'rohm_smplx_set_skinning': 'create-time upload of the skinning arrays into memory the handle owns',
    'rohm_posenet_exchange_status': 'status call: reads the exchange header of a workspace a forward of the same shape wrote; it is run '
                                    'after every PoseNet case as check_exchange',
    'rohm_posenet_set_stack_timeline': 'timeline call: registers a diagnostic output buffer; tests/test_gpu_chain.py checks its size',
}

# entry points that take a buffer but are not run by a case, each with its reason (at most these two: a third needs a sentence in the
# pull request that adds it saying why the contract does not apply)
EXEMPT = {
    'rohm_posenet_exchange_status': 'reads the exchange header by design (it is run after every PoseNet case as check_exchange, '
                                    'but what it reads is what the forward before it wrote)',
    'rohm_posenet_set_stack_timeline': 'a diagnostic OUTPUT buffer the kernel only writes stamps into; tests/test_gpu_chain.py '
                                       'checks it with a pre-filled buffer',
}

# case family (a prefix of case names in tests/test_gpu_stale_memory.py::CASES) -> the entry points its cases run
COVERAGE = {
    'gemm_res_layernorm': ['rohm_gemm_res_layernorm_f32'],
    'output_process': ['rohm_output_process_f32'],
    'attention': ['rohm_attention_f32'],
    'layernorm': ['rohm_layernorm_f32'],
    'planes': ['rohm_planes_split', 'rohm_gemm_planes', 'rohm_gemm_planes_ln', 'rohm_layernorm_planes_f32', 'rohm_attention_planes_f32'],
    'posenet_forward': ['rohm_posenet_forward'],
    'posenet_loop': ['rohm_posenet_sample_loop'],
    'posenet_guided': ['rohm_posenet_forward', 'rohm_guidance_skating_grad', 'rohm_ddpm_step_table'],
    'posenet_train': ['rohm_posenet_train_forward', 'rohm_posenet_train_backward'],
    'trajnet_forward': ['rohm_trajnet_forward'],
    'trajnet_loop': ['rohm_trajnet_sample_loop'],
    'trajnet_train': ['rohm_trajnet_train_forward', 'rohm_trajnet_train_backward'],
    'guidance_skating': ['rohm_guidance_skating_grad'],
    'guidance_skating_split': ['rohm_guidance_skating_prepare', 'rohm_guidance_skating_apply'],
    'guidance_proj2d': ['rohm_guidance_proj2d_grad'],
    'smplx_forward': ['rohm_smplx_forward'],
    'smplx_joints': ['rohm_smplx_joints'],
    'clips_build': ['rohm_clips_build'],
    'clips_build_f64': ['rohm_clips_build_f64'],
    'clips_repr': ['rohm_clips_repr'],
    'repr_stats': ['rohm_repr_stats'],
    'keypoints': ['rohm_keypoints_undistort', 'rohm_visibility_masks'],
    'depth': ['rohm_depth_render', 'rohm_depth_probe', 'rohm_project_pixels', 'rohm_joint_occlusion_mask'],
    'color': ['rohm_color_render', 'rohm_vertex_normals', 'rohm_skeleton_mesh'],
    'ddpm': ['rohm_ddpm_step', 'rohm_ddpm_step_table', 'rohm_posenet_dropout_mask'],
    'repr': ['rohm_smplx_frames_to_world', 'rohm_smplx_joints', 'rohm_repr_joints', 'rohm_repr_joints_vjp', 'rohm_traj_rederive'],
    'export_smplx': ['rohm_export_smplx'],
    'amass': ['rohm_amass_batch', 'rohm_smplx_param_noise', 'rohm_amass_preprocess'],
    'track_resample': ['rohm_track_resample'],
    'metrics': ['rohm_amass_metrics', 'rohm_scene_metrics', 'rohm_result_rows', 'rohm_traj_report'],
    'train_helpers': ['rohm_train_cond', 'rohm_train_traj_window', 'rohm_q_sample', 'rohm_image_requantize', 'rohm_image_paste',
                      'rohm_image_overlay', 'rohm_image_flip_lr'],
    'optim': ['rohm_grad_norm', 'rohm_adamw_step'],
    'multiview': ['rohm_mv_triangulate', 'rohm_mv_residuals'],
    'fit_views': ['rohm_fit_views_pose'],
    'rig': ['rohm_rig_pair_hypotheses', 'rohm_rig_pair_moments', 'rohm_rig_ba_moments', 'rohm_rig_ba_update'],
}


def covered_functions():
    return {f for fs in COVERAGE.values() for f in fs}
