"""The three launches on the LM loop's critical path -- trial_elim_kernel, bt_eliminate_tw_kernel<0>, bt_downsweep_kernel -- must keep
(a) no private segment: a per-lane array indexed at run time once put a store / load round trip through scratch memory in front of the
first column loads, and a private segment costs user SGPRs; (b) the leading flat arguments they declare preloaded into SGPRs: the
compiler preloads only a leading run of scalars and pointers, so one struct moved to the front silently turns the option into a no-op
(that is how a first experiment with it came to be recorded as useless).  Read from the gfx950 code objects of the built library: the
metadata notes and the kernel descriptors; no GPU needed."""
import os
import re
import struct
import subprocess
import tempfile

import pytest

from tests.test_codeobj_cpu import LIB, MAGIC, READELF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'islam_amd', 'csrc')
HIPCC = '/opt/rocm/bin/hipcc'
PRELOAD_OPT = ['-mllvm', '-amdgpu-kernarg-preload-count=16']
# kernel (a substring of its mangled name) -> the constant in the sources that declares its leading flat dwords (None: the kernel
# declares none and takes its struct first -- flat arguments in front of trial_elim_kernel's and bt_downsweep_kernel's structs were
# measured and did not shorten those kernels)
HOT = {'17trial_elim_kernel': None, '22bt_eliminate_tw_kernelILi0E': 'TW_FLAT_DWORDS', '19bt_downsweep_kernel': None}
# bytes 58..59 of the 64-byte kernel descriptor hold the kernarg preload spec: length in dwords (bits 0-6), offset (bits 7-15)
KD_PRELOAD_BYTE = 58

pytestmark = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(READELF)), reason='library or llvm-readelf missing')


def _readelf(*args):
    return subprocess.run([READELF, *args], capture_output=True, text=True, check=True).stdout


def _descriptors(co_path):
    """{kernel symbol: its 64-byte kernel descriptor} of one code object (the objects <kernel>.kd)"""
    sections = {}
    for m in re.finditer(r'^\s*\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)', _readelf('-W', '-S', co_path), re.M):
        sections[int(m.group(1))] = (int(m.group(3), 16), int(m.group(4), 16))          # index -> (address, file offset)
    data = open(co_path, 'rb').read()
    out = {}
    for m in re.finditer(r'^\s*\d+:\s+([0-9a-f]+)\s+64\s+OBJECT\s+\S+\s+\S+\s+(\d+)\s+(\S+)\.kd\s*$', _readelf('-W', '--symbols', co_path), re.M):
        addr, off = sections[int(m.group(2))]
        at = int(m.group(1), 16) - addr + off
        out[m.group(3)] = data[at:at + 64]
    return out


def _preload_length(kd):
    return struct.unpack_from('<H', kd, KD_PRELOAD_BYTE)[0] & 0x7f


@pytest.fixture(scope='module')
def library_kernels():
    """{kernel symbol: (metadata text, kernel descriptor)} over the gfx950 code objects bundled into the library"""
    data = open(LIB, 'rb').read()
    out, pos = {}, 0
    while True:
        i = data.find(MAGIC, pos)
        if i < 0:
            break
        pos = i + len(MAGIC)
        n, = struct.unpack_from('<Q', data, i + 24)
        off = i + 32
        for _ in range(n):
            o, s, ts = struct.unpack_from('<QQQ', data, off)
            off += 24
            triple = data[off:off + ts].decode()
            off += ts
            if 'gfx950' not in triple or s == 0:
                continue
            with tempfile.NamedTemporaryFile(suffix='.co') as f:
                f.write(data[i + o:i + o + s])
                f.flush()
                notes = _readelf('--notes', f.name)
                kds = _descriptors(f.name)
            for blk in notes.split('- .agpr_count')[1:]:
                m = re.search(r'\.name:\s+(\S+)', blk)
                if m and m.group(1) in kds:
                    out[m.group(1)] = (blk, kds[m.group(1)])
    return out


def _hot(library_kernels):
    found = {}
    for key in HOT:
        names = [k for k in library_kernels if key in k]
        assert len(names) == 1, (key, names)
        found[key] = library_kernels[names[0]]
    return found


def _declared(constant):
    """value of `constexpr int NAME = <sum of integers and other such constants>;` in the PVGO sources"""
    text = open(os.path.join(CSRC, 'pvgo_solver.inl')).read()
    m = re.search(r'constexpr int %s = ([A-Za-z_0-9 +]+);' % constant, text)
    assert m, constant
    return sum(int(t) if t.strip().isdigit() else _declared(t.strip()) for t in m.group(1).split('+'))


def test_hot_kernels_have_no_private_segment(library_kernels):
    for key, (blk, kd) in _hot(library_kernels).items():
        assert int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', blk).group(1)) == 0, key
        assert struct.unpack_from('<I', kd, 4)[0] == 0, key                  # the descriptor's own copy of the size


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc missing')
def test_descriptor_field_position_on_a_tiny_kernel(tmp_path):
    """six leading flat dwords in front of a struct: the assembler listing says so, and so must byte 58 of the descriptor"""
    src = tmp_path / 'tiny.hip'
    src.write_text('#include <hip/hip_runtime.h>\nstruct S { double a[4]; };\n'
                   'extern "C" __global__ void tiny(const double* x, int n, double* out, S s) { out[n] = x[n] + s.a[n & 3]; }\n'
                   'extern "C" __global__ void tiny_struct_first(S s, int n, double* out) { out[n] = s.a[n & 3]; }\n')
    base = [HIPCC, '-O3', '--offload-arch=gfx950', '--cuda-device-only', '--no-gpu-bundle-output', *PRELOAD_OPT, str(src)]
    subprocess.run(base + ['-S', '-o', str(tmp_path / 'tiny.s')], check=True, capture_output=True)
    subprocess.run(base + ['-c', '-o', str(tmp_path / 'tiny.co')], check=True, capture_output=True)
    listing = (tmp_path / 'tiny.s').read_text()
    want = {m.group(1): int(m.group(2)) for m in
            re.finditer(r'\.amdhsa_kernel (\w+)\n(?:.*\n)*?\s*\.amdhsa_user_sgpr_kernarg_preload_length (\d+)', listing)}
    assert want == {'tiny': 6, 'tiny_struct_first': 0}
    kds = _descriptors(str(tmp_path / 'tiny.co'))
    assert {k: _preload_length(kd) for k, kd in kds.items()} == want


def test_hot_kernels_preload_their_leading_flat_arguments(library_kernels):
    for key, (blk, kd) in _hot(library_kernels).items():
        # the leading run of pointers and 4-byte scalars in the metadata's argument list (a by-value struct ends it)
        args = [(int(o), int(s), k) for o, s, k in re.findall(r'- \.offset:\s+(\d+)\s+\.size:\s+(\d+)\s+\.value_kind:\s+(\w+)',
                                                               re.sub(r'\.(?:actual_access|address_space|access|name|type_name|is_const):\s+\S+\s+', '', blk))]
        assert args and args[0][0] == 0, key
        end = 0
        for o, s, k in args:
            if not (k == 'global_buffer' or (k == 'by_value' and s <= 8)):
                break
            end = o + s
        declared = _declared(HOT[key]) if HOT[key] else 0
        assert end == 4 * declared, (key, end, declared)
        assert declared <= 14 and (declared > 0 or HOT[key] is None), key
        assert _preload_length(kd) == declared, key
