// Test harness for ros/ with per-link depth thresholds: the adapter's sources against tests/ros_mock (NOT ROS), one model
// entry whose ~models[0]/link_depth_distance_thresholds names URDF links, and one 32FC1 frame through on_frame() with both
// outputs subscribed.  Shows that read_models() reads the array of {link, threshold} structs and that the filter applies it.
//   usage: ros_link_thresholds_harness urdf depth_file W H fx fy cx cy replace out_depth out_mask link threshold [link threshold ...]
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

#include "realtime_urdf_filter_amd_ros/ros_filter.hpp"
#include "../../ros/src/ros_filter.cpp"      // RosFilter::resolve_mesh (one translation unit: no library to link)

using namespace realtime_urdf_filter;

static std::string slurp(const char* path)
{
  std::ifstream f(path, std::ios::binary);
  return std::string((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv)
{
  if (argc < 14 || (argc - 12) % 2 != 0) { std::fprintf(stderr, "usage: see the head of %s\n", __FILE__); return 2; }
  const std::string xml = slurp(argv[1]), depth = slurp(argv[2]);
  const int W = std::atoi(argv[3]), H = std::atoi(argv[4]);
  if (depth.size() != (size_t)W * H * 4) { std::fprintf(stderr, "depth file has the wrong size\n"); return 2; }

  auto& P = ros::mock_parameter_server();
  P["~fixed_frame"] = "/world";
  P["~camera_frame"] = "/camera_rgb_optical_frame";
  P["~depth_distance_threshold"] = 0.05;
  P["~filter_replace_value"] = std::atof(argv[9]);
  P["~show_gui"] = false;
  XmlRpc::XmlRpcValue model;
  model["model"] = "robot_description"; model["tf_prefix"] = "/EXAMPLE"; model["geometry_type"] = "visual"; model["scale"] = 1;
  for (int i = 12, k = 0; i + 1 < argc; i += 2, k++) {
    model["link_depth_distance_thresholds"][k]["link"] = std::string(argv[i]);
    model["link_depth_distance_thresholds"][k]["threshold"] = std::atof(argv[i + 1]);
  }
  XmlRpc::XmlRpcValue models; models[0] = model;
  P["~models"] = models;
  P["/robot_description"] = xml;

  // tf: the link frames of the example under the prefix, the camera looking along world +y (as ros_adapter_harness.cpp)
  rtuf_host::StaticTransformProvider frames;
  for (const auto& kv : rtuf_host::forward_kinematics(rtuf_host::UrdfModel::from_string(xml))) frames.frames["/EXAMPLE/" + kv.first] = kv.second;
  frames.frames["/world"] = rtuf_host::Transform();
  rtuf_host::Transform cam;
  cam.m[0][0] = 1; cam.m[0][1] = 0; cam.m[0][2] = 0;
  cam.m[1][0] = 0; cam.m[1][1] = 0; cam.m[1][2] = 1;
  cam.m[2][0] = 0; cam.m[2][1] = -1; cam.m[2][2] = 0;
  frames.frames["/camera_rgb_optical_frame"] = cam;
  for (const auto& t : frames.frames)
    for (const auto& s : frames.frames) {
      rtuf_host::Transform x;
      frames.lookup(t.first, s.first, x);
      tf::StampedTransform st;
      for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) st.basis.m[r][c] = x.m[r][c];
      st.origin.v[0] = x.o.x; st.origin.v[1] = x.o.y; st.origin.v[2] = x.o.z;
      tf::mock_transforms()[{t.first, s.first}] = st;
    }

  ros::NodeHandle nh("~");
  try {
    RosFilter filter(nh, argc, argv);
    auto& topics = image_transport::mock_topics();
    if (!topics.count("input_depth") || !topics["input_depth"].callback) { std::fprintf(stderr, "the adapter did not subscribe to input_depth\n"); return 1; }
    topics["output_depth"].subscribers = 1;
    topics["output_mask"].subscribers = 1;
    auto image = boost::make_shared<sensor_msgs::Image>();
    image->header.stamp = ros::Time(12.5); image->header.frame_id = "/camera_rgb_optical_frame";
    image->width = (uint32_t)W; image->height = (uint32_t)H; image->encoding = "32FC1"; image->is_bigendian = 0;
    image->step = (uint32_t)((size_t)W * 4);
    image->data.assign(depth.begin(), depth.end());
    auto info = boost::make_shared<sensor_msgs::CameraInfo>();
    info->width = (uint32_t)W; info->height = (uint32_t)H;
    info->P[0] = std::atof(argv[5]); info->P[5] = std::atof(argv[6]); info->P[2] = std::atof(argv[7]); info->P[6] = std::atof(argv[8]); info->P[10] = 1;
    topics["input_depth"].callback(image, info);

    for (const std::string& l : ros::mock_log()) std::printf("log %s\n", l.c_str());
    const auto& dp = topics["output_depth"].published; const auto& mp = topics["output_mask"].published;
    std::printf("published depth %zu mask %zu\n", dp.size(), mp.size());
    if (dp.size() != 1u || mp.size() != 1u) return 1;
    std::ofstream(argv[10], std::ios::binary).write(reinterpret_cast<const char*>(dp[0].first->data.data()), (std::streamsize)dp[0].first->data.size());
    std::ofstream(argv[11], std::ios::binary).write(reinterpret_cast<const char*>(mp[0].first->data.data()), (std::streamsize)mp[0].first->data.size());
  } catch (const std::exception& e) {
    std::printf("error %s\n", e.what());
    return 3;
  }
  return 0;
}
