"""The detail joints (decoder.hip: joint_argmax_update<., true> in dec_joint_kernel<true> and
dec_joint_slim_kernel<true>) on the host emulation of the wave model (tools/emu, detail mode): the
per-token emission frames and confidences equal, bit for bit, a host replay of the greedy loop over
oracle_prediction / oracle_joint / oracle_exp -- Offline (one call) and the Server form (two calls
over the halves of the frames: the slots' frame base carries), in both kernel families, with the
bounds checks on and nothing written at or past res_len.  No GPU."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if not os.path.exists(CLANG) or not shutil.which("python3"):
        pytest.skip("no ROCm clang++")
    out = tmp_path_factory.mktemp("emu_detail")
    env = dict(os.environ, EMU_ASAN="0", EMU_OUT=str(out), EMU_CFLAGS="-DRNNT_DEV_KNOBS")  # RNNT_DEC_SLIM below
    subprocess.run(["bash", os.path.join(REPO, "tools", "emu", "build.sh")], check=True, env=env,
                   capture_output=True, timeout=600)
    return str(out / "dec_emu")


def _check(r):
    assert r.returncode == 0, r.stdout + r.stderr
    for line in ("bounds checks: ok", "tokens identical", "frames identical", "conf identical",
                 "positions past res_len: untouched"):
        assert line in r.stdout, r.stdout


@pytest.mark.parametrize("server", [0, 1])
@pytest.mark.parametrize("slim", ["15", "0"])
def test_detail_joints_match_the_replay_on_the_emulator(emu, server, slim):
    # slim 15: the co-resident step kernels (the default), 0: the big-tile step kernels
    r = subprocess.run([emu, "6", "4", "5", str(server), "12", "1"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, RNNT_DEC_SLIM=slim))
    _check(r)


def test_detail_joint_walks_several_tiles_on_the_emulator(emu):
    # 40 rows, one row group per kernel: one joint workgroup walks three 16-row tiles
    r = subprocess.run([emu, "40", "6", "5", "0", "12", "1"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, RNNT_DEC_RG="1x1x1"))
    _check(r)


def test_five_argument_invocation_is_unchanged(emu):
    r = subprocess.run([emu, "6", "4", "5", "0", "12"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tokens identical" in r.stdout and "bounds checks: ok" in r.stdout
    assert "frames" not in r.stdout and "conf" not in r.stdout, r.stdout
