"""The C++ shims of include/shims/ are real code: they compile (-Wall -Werror) against ONE set of minimal mock OpenCV / ORB-SLAM2
headers (tests/mock_orbslam/, test infrastructure) with the helper header include/shims/orbfe_shim.h, link against liborbfe.so --
each with its driver, and all of them into one program, as an integration links them -- and without a GPU the driver stops at the
library's loud "no device" answer instead of falling back to anything."""
import os
import subprocess

import pytest

import shim_build

SHIM_PROGRAMS = ["matcher", "init", "pose", "sim3", "sim3_opt", "kfdb"]


def _library():
    from orb_slam2_aruco_amd import binding
    if not os.path.exists(binding.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


@pytest.mark.parametrize("name", SHIM_PROGRAMS)
def test_shim_compiles_and_links_against_the_mock_headers(name, tmp_path):
    """every shim with the reference's signatures and its driver: g++ -Wall -Werror, linked against liborbfe.so"""
    assert sorted(SHIM_PROGRAMS + ["all"]) == sorted(shim_build.PROGRAMS)
    _library()
    assert os.path.exists(shim_build.build(name, str(tmp_path)))


def test_all_shims_compile_and_link_into_one_program(tmp_path):
    """the eleven .cc shims, the two header shims and every mock class header in one program (tests/all_shims_driver.cpp): one Frame,
    KeyFrame, MapPoint and Optimizer declaration serves them all, and no symbol is defined twice.  The program opens no device."""
    _library()
    exe = shim_build.build("all", str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("ok: 11 shims")


def test_shims_compile_link_and_refuse_without_a_gpu(tmp_path):
    from orb_slam2_aruco_amd import binding
    exe = shim_build.build("matcher", str(tmp_path))
    if binding.load().orbfe_device_count() > 0:
        pytest.skip("a GPU is present: tests/test_shims_gpu.py runs the driver")
    r = subprocess.run([exe, "none", "1", "1", "1", str(tmp_path / "o")], capture_output=True, text=True)
    assert r.returncode == 3 and "no HIP device" in r.stderr


def test_shim_headers_declare_the_reference_interfaces():
    """Signatures the call sites of the reference need (ORBextractor.h:59-83, markerdetector.h:222-312, ORBmatcher.h:44-83)."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ex = open(os.path.join(root, "include", "shims", "ORBextractor.h")).read()
    for sig in ("ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST)",
                "void operator()(cv::InputArray _image, cv::InputArray /*_mask*/, std::vector<cv::KeyPoint>& _keypoints, cv::OutputArray _descriptors)",
                "GetLevels()", "GetScaleFactor()", "GetScaleFactors()", "GetInverseScaleFactors()", "GetScaleSigmaSquares()",
                "GetInverseScaleSigmaSquares()", "std::vector<cv::Mat> mvImagePyramid"):
        assert sig in ex, sig
    md = open(os.path.join(root, "include", "shims", "MarkerDetector.h")).read()
    for sig in ("MarkerDetector(std::string dict_type, float error_correction_rate = 0)",
                "void setDictionary(std::string dict_type, float error_correction_rate = 0)",
                "void setDetectionMode(DetectionMode dm, float minMarkerSize = 0)", "Params& getParameters()",
                "std::vector<aruco::Marker> detect(const cv::Mat& input)",
                "std::vector<aruco::Marker> detect(const cv::Mat& input, const CameraParameters& camParams, float markerSizeMeters,",
                "void detect(const cv::Mat& input, std::vector<Marker>& detectedMarkers, CameraParameters camParams, float markerSizeMeters = -1,",
                "void detect(const cv::Mat& input, std::vector<Marker>& detectedMarkers, cv::Mat camMatrix = cv::Mat(), cv::Mat distCoeff = cv::Mat(),"):
        assert sig in md, sig
    om = open(os.path.join(root, "include", "shims", "ORBmatcher_orbfe.cc")).read()
    for name in ("DescriptorDistance", "SearchByProjection(Frame& F, const vector<MapPoint*>& vpMapPoints",
                 "SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame", "SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF",
                 "SearchByProjection(KeyFrame* pKF, cv::Mat Scw", "SearchByBoW(KeyFrame* pKF, Frame& F", "SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2",
                 "SearchForInitialization(Frame& F1, Frame& F2", "SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2", "SearchBySim3(KeyFrame* pKF1",
                 "Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints", "Fuse(KeyFrame* pKF, cv::Mat Scw"):
        assert "ORBmatcher::" + name in om, name
