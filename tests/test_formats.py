"""The format descriptions and option checks (`lut_renderer_amd.formats`) stand without torch: the argv builder and the numpy
container helpers import them, and `engine_command` renders every engine option, in a process that never loads torch."""
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent

# (the argument values are those of test_dual.py, test_chain.py and test_premul.py's engine_command cases)
_CHILD = r"""
import sys
from pathlib import Path
import lut_renderer_amd.formats, lut_renderer_amd.command, lut_renderer_amd.semiplanar, lut_renderer_amd.packedyuv, lut_renderer_amd.v210
from lut_renderer_amd.command import _master_params, engine_command
from lut_renderer_amd.params import ProcessingParams, VideoInfo

info = VideoInfo(width=1920, height=1080, bit_depth=10, pix_fmt="yuv420p10le", color_range="tv", colorspace="bt709", fps=25.0,
                 duration=4.0)
master = _master_params(ProcessingParams(video_codec="libx264", crf="18"))
dual = engine_command(Path("-"), Path("-"), master, Path("look.cube"), info, python_bin="python3",
                      second_output=Path("delivery.yuv"), second_pix_fmt="yuv420p")
assert dual[-4:] == ["--second-output", "delivery.yuv", "--second-pix-fmt", "yuv420p"], dual
chain = engine_command(Path("-"), Path("-"), ProcessingParams(video_codec="libx265", pix_fmt="yuv420p10le"), Path("tech.cube"), info,
                       python_bin="python3", cube2=Path("look.cube"), interp2="trilinear")
assert chain[-4:] == ["--cube2", "look.cube", "--interp2", "trilinear"], chain
yuva = VideoInfo(width=64, height=36, bit_depth=10, pix_fmt="yuva444p10le", fps=25.0)
premul = engine_command(Path("-"), Path("-"), ProcessingParams(video_codec="prores_ks", pix_fmt="yuva444p10le"), "look.cube", yuva,
                        python_bin="python", alpha_mode="premultiplied")
assert premul[-2:] == ["--alpha-mode", "premultiplied"], premul
assert "torch" not in sys.modules, sorted(m for m in sys.modules if m.startswith("torch"))[:5]
print("TORCH_FREE")
"""


def test_formats_and_the_argv_builder_never_load_torch():
    done = subprocess.run([sys.executable, "-c", _CHILD], cwd=str(ROOT), capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    assert done.stdout.strip().endswith("TORCH_FREE")
