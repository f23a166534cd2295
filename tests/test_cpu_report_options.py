"""CPU: --no-psnr, --no-ssim, --quiet and -v reach the encoder (x264's defaults measure both, R/common/common.c:131-132), and the lossless rule of
x264_validate_parameters (R/encoder/encoder.c:410-411) holds on the way."""
from x264_vs2008_amd import encode as E
from x264_vs2008_amd import slice as sl


def fields(args):
    o = E.build_parser().parse_args(args.split() + ["-o", "x.264", "in_96x80.yuv"])
    E.param_fields(o)                                    # (none of these options is a stream parameter: the stream's fields parse as before)
    return E.report_fields(o)


def test_report_options_reach_the_encoder_parameters():
    assert fields("--qp 26") == dict(psnr=1, ssim=1, verbose=False, quiet=False)
    assert fields("--qp 26 --no-psnr") == dict(psnr=0, ssim=1, verbose=False, quiet=False)
    assert fields("--qp 26 --no-ssim -v") == dict(psnr=1, ssim=0, verbose=True, quiet=False)
    assert fields("--qp 26 --verbose --no-psnr --no-ssim") == dict(psnr=0, ssim=0, verbose=True, quiet=False)
    assert fields("--qp 26 --quiet -v") == dict(psnr=0, ssim=0, verbose=False, quiet=True)


def test_flags_follow_the_options():
    from x264_vs2008_amd import quality as q
    assert q.flags(1, 1, 2) == q.REPORT_PSNR | q.REPORT_SSIM | q.REPORT_REFS and q.flags(0, 1, 1) == q.REPORT_SSIM and q.flags(0, 0, 1) == 0
    import inspect
    sig = inspect.signature(sl.ChainEncoder.__init__).parameters
    assert sig["psnr"].default == 0 and sig["ssim"].default == 0 and sig["mb_stats"].default == 0          # off unless asked for: nothing is enqueued
