"""Optional rclpy glue around seam B3: a ROS 2 node with the reference PoseNode's topics whose pose comes from `gisnav_amd.pose_node.PoseNode`.

The reference node (ros/gisnav/gisnav/core/pose_node.py) subscribes to `/camera/camera_info` (constants.py:69) and to StereoNode's
`/gisnav/stereo_node/pose_image` (OrthoStereoImage; pose_node.py:499-505).  From the solver's (r, t) it forms the pose of `camera_optical` in the
REP 105 `earth` frame (pose_node.py:333-381) and then walks the tf tree (gisnav_map <- earth, camera_link_optical -> base_link: pose_node.py:383-470)
to publish `~/pose` in `gisnav_map`.  This module is the MINIMAL node: same two subscriptions, and the EARTH-frame camera pose on `~/pose_earth`
(PoseWithCovarianceStamped, frame_id "earth") -- everything up to pose_node.py:381.  The tf2 buffer / broadcasters, the debug images
(pose_node.py:310-347) and the EKF `set_pose` client (pose_node.py:136-163) are the ROS control plane and stay with the reference: a deployment
that wants the complete node applies INTEGRATION.md 2's two-line edit to the reference's own PoseNode, which keeps all of it.  What runs here:

    ROS messages -> `gisnav_amd.wire` dataclasses (the bytes of `query_sift.data` untouched, the mono8 rasters as numpy views)
                 -> `PoseNode.estimate` (matcher + DEM lift + PnP on the GPU: pose_node.py:207-308)
                 -> `georef.pose_to_earth` (pose_node.py:333-381: camera position through the CRS affine to WGS 84 to ECEF, orientation ENU -> ECEF)
                 -> PoseWithCovarianceStamped, stamped like pose_node.py:489-495, `pose.covariance` from the PnP inliers (`fill_pose_message`)

rclpy, sensor_msgs, geometry_msgs and gisnav_msgs are NOT part of this repository's image: importing this module always works, building the node
class needs them (`make_node_class()` raises ImportError naming what is missing).  The message conversion is plain Python on duck-typed
messages and is tested on the CPU (tests/test_ros2_glue.py)."""
from __future__ import annotations

from typing import Any, Optional

import numpy as np

from .wire import CameraInfo, ImageMsg, OrthoStereoImage, Stamp

ROS_TOPIC_CAMERA_INFO = "/camera/camera_info"                 # constants.py:69
ROS_TOPIC_POSE_IMAGE = "/gisnav/stereo_node/pose_image"       # f"/{ROS_NAMESPACE}/" + ROS_TOPIC_RELATIVE_POSE_IMAGE.replace("~", STEREO_NODE_NAME): pose_node.py:500-503
ROS_TOPIC_POSE_EARTH = "~/pose_earth"                         # (the reference's `~/pose`, constants.py:64, is the tf-chained gisnav_map pose: not published here)


def _stamp(header: Any) -> Stamp:
    s = header.stamp
    return Stamp(int(s.sec), int(s.nanosec))


def image_to_mono8(img: Any) -> np.ndarray:
    """sensor_msgs/Image (mono8) -> (height, width) uint8 view of its data, honouring `step` (what `CvBridge.imgmsg_to_cv2(msg, "mono8")` returns for
    a mono8 image: pose_node.py:216, 221-223).  Other encodings are refused: StereoNode publishes mono8 rasters (stereo_node.py:262-275)."""
    if getattr(img, "encoding", "mono8") not in ("mono8", "8UC1"):
        raise ValueError(f"expected a mono8 raster, got encoding {img.encoding!r}")
    h, w = int(img.height), int(img.width)
    step = int(getattr(img, "step", w)) or w
    buf = np.frombuffer(bytes(img.data) if not isinstance(img.data, (bytes, bytearray, memoryview, np.ndarray)) else img.data, dtype=np.uint8)
    if buf.size < h * step:
        raise ValueError("image data shorter than height x step")
    return buf[: h * step].reshape(h, step)[:, :w]


# sensor_msgs/Image encodings of an elevation raster -> numpy element type (GN_DEM_U8 / U16 / I16 / F32)
DEM_ENCODINGS = {"mono8": "u1", "8UC1": "u1", "mono16": "u2", "16UC1": "u2", "16SC1": "i2", "32FC1": "f4"}


def image_to_dem(img: Any) -> np.ndarray:
    """sensor_msgs/Image holding an elevation raster -> (height, width) array of its element type: mono8 / 8UC1 uint8, mono16 / 16UC1 uint16,
    16SC1 int16, 32FC1 float32, in native byte order.  Honours `step` (bytes per row, which may exceed width x element size) and `is_bigendian`.
    Any other encoding is refused by name."""
    enc = getattr(img, "encoding", "mono8")
    if enc not in DEM_ENCODINGS:
        raise ValueError(f"expected an elevation raster of encoding {', '.join(DEM_ENCODINGS)}, got encoding {enc!r}")
    dt = np.dtype(DEM_ENCODINGS[enc]).newbyteorder(">" if getattr(img, "is_bigendian", 0) else "<")
    h, w = int(img.height), int(img.width)
    step = int(getattr(img, "step", w * dt.itemsize)) or w * dt.itemsize
    if step < w * dt.itemsize:
        raise ValueError(f"image step {step} is shorter than a row of {w} {enc} elements")
    buf = np.frombuffer(bytes(img.data) if not isinstance(img.data, (bytes, bytearray, memoryview, np.ndarray)) else img.data, dtype=np.uint8)
    if buf.size < h * step:
        raise ValueError("image data shorter than height x step")
    rows = buf[: h * step].reshape(h, step)[:, : w * dt.itemsize]
    if dt.itemsize == 1:
        return rows
    out = np.ascontiguousarray(rows).view(dt).reshape(h, w)
    return out if dt.isnative else out.astype(dt.newbyteorder("="))


def ortho_stereo_image_from_ros(msg: Any) -> OrthoStereoImage:
    """gisnav_msgs/OrthoStereoImage -> the wire dataclass `PoseNode.estimate` takes.  `query_sift.data` is passed on as bytes: the 532-byte
    KEYPOINT_DTYPE records go to the device as they are."""
    data = msg.query_sift.data
    raw = data.tobytes() if hasattr(data, "tobytes") else bytes(data)
    q_stamp = _stamp(msg.query.header)
    if q_stamp.sec == 0:                                       # pose_node.py:489-495: an empty query image carries no stamp, the keypoint cloud does
        q_stamp = _stamp(msg.query_sift.header)
    return OrthoStereoImage(query_sift=raw,
                            reference=ImageMsg(image_to_mono8(msg.reference), _stamp(msg.reference.header)),
                            dem=ImageMsg(image_to_dem(msg.dem), _stamp(msg.dem.header)),      # (the raster keeps its element type)
                            crs=str(msg.crs.data), query_stamp=q_stamp)


def camera_info_from_ros(msg: Any) -> CameraInfo:
    """sensor_msgs/CameraInfo -> the wire dataclass, `d` and `distortion_model` included (read only with use_distortion=True)."""
    d = getattr(msg, "d", None)
    return CameraInfo(k=np.asarray(msg.k, np.float64).reshape(9), height=int(msg.height), width=int(msg.width),
                      d=None if d is None else np.asarray(d, np.float64).reshape(-1), distortion_model=str(getattr(msg, "distortion_model", "") or ""))


def pose_fields(r: np.ndarray, t: np.ndarray, crs: str, ref_shape, cov_rt: Optional[np.ndarray] = None) -> Optional[dict]:
    """(r, t) of the solver -> the fields of the published pose: ECEF position, (x, y, z, w) orientation (pose_node.py:333-381); None when the
    camera centre falls outside the reference raster (pose_node.py:341-343).  cov_rt (PoseNode.last_covariance) adds "covariance": the 6x6
    earth-frame covariance in the order of geometry_msgs/PoseWithCovariance."""
    from .georef import pose_to_earth
    return pose_to_earth(r, t, crs, ref_shape, cov_rt=cov_rt)


def fill_pose_message(out: Any, fields: dict, stamp: Stamp, frame_id: str = "earth") -> Any:
    """Fill a (duck-typed) geometry_msgs/PoseWithCovarianceStamped from `pose_fields`' result: header, position, orientation, and
    `pose.covariance` as 36 row-major floats (x, y, z, rotation about the fixed X, Y, Z axes) when the fields carry a covariance.  Without
    one -- the solver's cov_ok was 0, or the node does not ask for it -- the message's covariance is left as it was constructed: all zeros."""
    out.header.frame_id = frame_id
    out.header.stamp.sec, out.header.stamp.nanosec = stamp.sec, stamp.nanosec
    p, q = fields["position"], fields["orientation"]
    out.pose.pose.position.x, out.pose.pose.position.y, out.pose.pose.position.z = float(p[0]), float(p[1]), float(p[2])
    o = out.pose.pose.orientation
    o.x, o.y, o.z, o.w = float(q[0]), float(q[1]), float(q[2]), float(q[3])
    cov = fields.get("covariance")
    if cov is not None:
        out.pose.covariance = [float(v) for v in np.asarray(cov, np.float64).reshape(36)]
    return out


def make_node_class():
    """Build the rclpy Node subclass (import-guarded: rclpy and the message packages are absent from this repository's image)."""
    try:
        import rclpy  # noqa: F401
        from rclpy.node import Node
        from rclpy.qos import QoSPresetProfiles
        from geometry_msgs.msg import PoseWithCovarianceStamped
        from sensor_msgs.msg import CameraInfo as RosCameraInfo
        from gisnav_msgs.msg import OrthoStereoImage as RosOrthoStereoImage
    except ImportError as exc:  # pragma: no cover - exercised by tests through the message below
        raise ImportError("gisnav_amd.ros2_node needs a ROS 2 environment (rclpy, sensor_msgs, geometry_msgs, gisnav_msgs): " + str(exc)) from exc

    from .pose_node import PoseNode

    class GisnavAmdPoseNode(Node):
        """`~/pose_earth` from `/camera/camera_info` + StereoNode's pose image, computed by gisnav_amd (one message = one GPU call, ~1 ms)."""

        def __init__(self, state_dict, *args, device: int = 0, precision: str = "f16x2_f16_attn", use_distortion: bool = False,
                     ransac_iterations: int = 10, report: bool = False, dem_scale: float = 1.0, dem_offset: float = 0.0, dem_nodata=None, **kwargs):
            super().__init__(*args, **kwargs)
            # report=True: `last_report` holds the matches, cv2-style inliers and residuals of the most recent message (PoseNode.last_report)
            self._impl = PoseNode(state_dict, device=device, precision=precision, covariance=True, use_distortion=use_distortion,
                                  ransac_iterations=ransac_iterations, report=report,
                                  dem_scale=dem_scale, dem_offset=dem_offset, dem_nodata=dem_nodata)
            self._camera_info: Optional[CameraInfo] = None
            qos = QoSPresetProfiles.SENSOR_DATA.value
            self._pub = self.create_publisher(PoseWithCovarianceStamped, ROS_TOPIC_POSE_EARTH, qos)
            self.create_subscription(RosCameraInfo, ROS_TOPIC_CAMERA_INFO, self._camera_info_cb, qos)
            self.create_subscription(RosOrthoStereoImage, ROS_TOPIC_POSE_IMAGE, self._pose_image_cb, qos)

        @property
        def last_report(self) -> Optional[dict]:
            return self._impl.last_report

        def _camera_info_cb(self, msg) -> None:
            self._camera_info = camera_info_from_ros(msg)

        def _pose_image_cb(self, msg) -> None:
            if self._camera_info is None:                      # narrow_types: no result until both inputs exist (_decorators.py:117-160)
                return
            # one malformed message (a non-mono8 raster, a short keypoint buffer, more keypoints than the context can grow to) must not kill the node:
            # exceptions of the conversion and of the estimator are logged and the message is dropped
            try:
                wire = ortho_stereo_image_from_ros(msg)
                pose = self._impl.estimate(self._camera_info, wire)
            except Exception as exc:  # noqa: BLE001
                self.get_logger().warning(f"pose_image message dropped: {exc.__class__.__name__}: {exc}")
                return
            if pose is None:
                self.get_logger().warning(f"no pose ({self._impl.last_num_matches} matches)")
                return
            fields = pose_fields(pose[0], pose[1], wire.crs, wire.reference.data.shape, cov_rt=self._impl.last_covariance)
            if fields is None:
                self.get_logger().warning("camera centre outside the reference raster - no pose")
                return
            # pose.covariance: the first-order covariance of the PnP estimate pushed to the earth frame (the reference leaves it all-zero:
            # pose_node.py:477 "TODO: re-enable covariance/implement error model"); zeros remain only when the solver reports cov_ok = 0
            self._pub.publish(fill_pose_message(PoseWithCovarianceStamped(), fields, wire.query_stamp))

    return GisnavAmdPoseNode
