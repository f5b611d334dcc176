"""Static check of the built library (no GPU): the kernel families built without packed fp32 arithmetic.

csrc/Makefile builds the objects of UNPACKED without the SLP vectoriser, which under plain -O3 packs adjacent scalar fp32
operations into v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 and assembles their register pairs with extra moves.  On
gfx950 the packed forms have the rate of the scalar ones and cost more beside other waves' matrix instructions; for
dp_bwd16s they also cost 55 registers, which the kernel now uses to keep its tables and lane indices (DESIGN.md section 10,
profiles/unpacked_fp32.json).

The test takes the device code objects out of libyunet_hip.so with the ROCm llvm-objdump, reads every kernel's metadata
with llvm-readelf and disassembles it.  Every instance of an ADOPTED family holds none of the three packed operations,
spills no register and has no private segment.  LEFT_PACKED lists the families that keep the compiler's packing, with the
measurement that decided it (per-launch times inside the training step, 256 images at 320 x 320, parent -> unpacked).
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'libfacedetection.train_amd', 'libyunet_hip.so')
LLVM = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin')
OBJDUMP = shutil.which('llvm-objdump', path=LLVM) or shutil.which('llvm-objdump')
READELF = shutil.which('llvm-readelf', path=LLVM) or shutil.which('llvm-readelf')

# family (substring of the mangled kernel name) -> number of instances in the library: fp32 storage <POOLDY, DET> x 4,
# bf16 storage <POOLDY> x 2 (the deterministic forms exist for fp32 storage only)
ADOPTED = {'dp_bwd16s_kernel': 6}
LEFT_PACKED = {
    'dp_bwd64_kernel': 'no faster unpacked: <8,true,false> 0.308 -> 0.322 ms, <8,false,false> 0.392 -> 0.401 ms, the others unchanged',
    'dp_fwd64s_kernel': 'slower unpacked: <false> 0.473 -> 0.483 ms, <true> 0.253 -> 0.259 ms',
    'dp_fwd16s_kernel': 'instances disagree: <16,true> 0.182 -> 0.175 ms, <64,false> 0.144 -> 0.149 ms',
    'dp_bwd_kernel': 'slower unpacked: <16,64,...> 0.328 -> 0.336 ms; 20 of 46 instances go to 256 registers and spill',
    'stem_mma_kernel': 'no faster unpacked: <false> 0.135 -> 0.140 ms, <true> unchanged',
    'dp_fwd_kernel': 'unchanged within the noise of the measurement (0.053 -> 0.052 ms)',
}
PACKED = re.compile(r'\bv_pk_(fma|mul|add)_f32\b')

pytestmark = pytest.mark.skipif(not (OBJDUMP and READELF), reason='ROCm llvm-objdump / llvm-readelf not found')


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    """{(code object, kernel symbol): {'packed': n, 'spill': spilled VGPRs, 'private': bytes}} of every kernel of the library."""
    assert os.path.exists(LIB), 'build the library first (python __graft_entry__.py)'
    tmp = tmp_path_factory.mktemp('codeobj')
    lib = shutil.copy(LIB, tmp / 'lib.so')                # llvm-objdump writes the bundles next to its input
    subprocess.run([OBJDUMP, '--offloading', lib], check=True, capture_output=True, cwd=tmp, timeout=120)
    out = {}
    for co in sorted(f for f in os.listdir(tmp) if 'gfx950' in f):
        path = str(tmp / co)
        notes = subprocess.run([READELF, '--notes', path], check=True, capture_output=True, text=True, timeout=120).stdout
        for blk in re.split(r'\n\s+- \.agpr_count:', notes)[1:]:
            def field(key):
                return re.search(r'\.' + key + r':\s+(\S+)', blk).group(1)
            out[(co, field('symbol')[:-len('.kd')])] = {'packed': 0, 'spill': int(field('vgpr_spill_count')),
                                        'private': int(field('private_segment_fixed_size'))}
        asm = subprocess.run([OBJDUMP, '-d', path], check=True, capture_output=True, text=True, timeout=300).stdout
        sym = None
        for line in asm.splitlines():
            m = re.match(r'[0-9a-f]+ <(\S+)>:', line)
            if m:
                sym = (co, m.group(1))
            elif sym in out and PACKED.search(line):
                out[sym]['packed'] += 1
    assert out, 'no gfx950 kernel found in the library'
    return out


@pytest.mark.parametrize('family', sorted(ADOPTED))
def test_adopted_family_is_unpacked_and_free_of_scratch(kernels, family):
    inst = {k: v for k, v in kernels.items() if family in k[1]}
    assert len(inst) == ADOPTED[family], sorted(inst)
    for key, v in inst.items():
        assert v['packed'] == 0, (key, v)
        assert v['spill'] == 0 and v['private'] == 0, (key, v)


def test_families_left_packed_are_kernels_of_the_library(kernels):
    names = ' '.join(k[1] for k in kernels)
    for family, reason in LEFT_PACKED.items():
        assert family in names and family not in ADOPTED and reason, family
