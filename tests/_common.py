"""What the test modules share (a plain module, imported by name): the tensor, pointer, numpy and stream helpers of the callers of the
library's entries, the first argmin of the nearest-prior statements, and the build-and-run of a stand-alone sanitizer program."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'anytime-3d-reconstruction_amd')


def _t(x, device):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _np(t, bf16_bits=False):
    """A tensor as numpy; a bfloat16 one as its float32 values or, with bf16_bits, as its raw uint16."""
    if t.dtype != torch.bfloat16:
        return t.cpu().numpy()
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if bf16_bits else t.float().cpu().numpy()


def _stream(device):
    return [] if device == 'cpu' else [ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)]


def first_argmin(d):
    """First argmin among the distances below +inf; a row without one gets 0."""
    ok = d < np.inf
    return np.where(ok.any(axis=-1), np.argmin(np.where(ok, d, np.inf), axis=-1), 0).astype(np.int32)


def build_and_run_sanitized(main_cpp, tmp_path, name):
    """tests/<main_cpp> with the headers of csrc/ as ONE program of its own (tmp_path/<name>) under the address and undefined-behaviour
    sanitizers, built by the first compiler that can and run on the CPU: it must exit 0, end its output with OK and report nothing."""
    from voxvae import build as vb
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(vb.HIPCC))), 'llvm', 'bin', 'clang++')
    compilers = [c for c in (rocm_clang, shutil.which('clang++'), shutil.which('g++')) if c and os.path.exists(c)]
    assert compilers, 'no C++ compiler found'
    exe, log = str(tmp_path / name), ''
    for cxx in compilers:
        r = subprocess.run([cxx, '-x', 'c++', '-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer', '-fsanitize=address,undefined',
                            '-fno-sanitize-recover=all', '-I', os.path.join(PKG, 'csrc'), os.path.join(ROOT, 'tests', main_cpp),
                            '-o', exe, '-lm'], capture_output=True, text=True)
        log += '%s: %s\n' % (cxx, r.stderr[-2000:])
        if r.returncode == 0:
            break
    else:
        pytest.fail('no compiler built the sanitizer program:\n' + log)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith('OK'), r.stdout[-2000:] + r.stderr[-4000:]
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr
