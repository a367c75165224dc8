// ear/metadata.hpp — the metadata the gain producers read: type names, field names and defaults of libear's
// DirectSpeakersTypeMetadata, ObjectsTypeMetadata and HOATypeMetadata (include/ear/metadata.hpp:11-171).  libear's
// boost::variant members (position, objectDivergence, exclusion zones, the DirectSpeakers position) are plain structs
// here that convert from the same alternative types, and its boost::optional members are ear::Optional, so the lines
// a libear application writes — `otm.position = PolarPosition(...)`, `otm.objectDivergence =
// PolarObjectDivergence(0.5)`, `zones.push_back(PolarExclusionZone{...})`, `pos.azimuthMin = 0.0`,
// `dstm.audioPackFormatID = "AP_00010002"` — compile unchanged.
#pragma once
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "layout.hpp"
#include "screen.hpp"

namespace ear {
  /// what libear's metadata holds as boost::optional<T>: empty by default, set by assigning a value; read with
  /// `if (o)`, `*o` / get() and value_or
  template <typename T>
  class Optional {
   public:
    Optional() = default;
    template <typename U, typename = typename std::enable_if<std::is_convertible<U, T>::value>::type>
    Optional(U &&value) : has_(true), value_(std::forward<U>(value)) {}
    explicit operator bool() const { return has_; }
    const T &get() const {
      if (!has_) throw internal_error("an empty optional was read");
      return value_;
    }
    const T &operator*() const { return get(); }
    T value_or(const T &other) const { return has_ ? value_ : other; }
    void reset() { has_ = false, value_ = T(); }

   private:
    bool has_ = false;
    T value_ = T();
  };

  // typeDefinition == DirectSpeakers (include/ear/metadata.hpp:11-71)

  /// the `screenEdgeLock` attributes of the position elements (azimuth / X and elevation / Z)
  struct ScreenEdgeLock {
    Optional<std::string> horizontal;
    Optional<std::string> vertical;
  };
  struct PolarSpeakerPosition {
    PolarSpeakerPosition(double az = 0.0, double el = 0.0, double dist = 1.0) : azimuth(az), elevation(el), distance(dist) {}
    double azimuth;
    Optional<double> azimuthMin;
    Optional<double> azimuthMax;
    double elevation;
    Optional<double> elevationMin;
    Optional<double> elevationMax;
    double distance;
    Optional<double> distanceMin;
    Optional<double> distanceMax;
    ScreenEdgeLock screenEdgeLock;
  };
  /// (refused by ear::GainCalculatorDirectSpeakers, as in libear; ear::hip::DirectSpeakersGainCalculator takes it)
  struct CartesianSpeakerPosition {
    CartesianSpeakerPosition(double X = 0.0, double Y = 1.0, double Z = 0.0) : X(X), Y(Y), Z(Z) {}
    double X;
    Optional<double> XMin;
    Optional<double> XMax;
    double Y;
    Optional<double> YMin;
    Optional<double> YMax;
    double Z;
    Optional<double> ZMin;
    Optional<double> ZMax;
    ScreenEdgeLock screenEdgeLock;
  };
  /// libear: boost::variant<PolarSpeakerPosition, CartesianSpeakerPosition>
  struct SpeakerPosition {
    SpeakerPosition(PolarSpeakerPosition p = PolarSpeakerPosition()) : isCartesian(false), polar(std::move(p)) {}
    SpeakerPosition(CartesianSpeakerPosition c) : isCartesian(true), cartesian(std::move(c)) {}
    bool isCartesian;
    PolarSpeakerPosition polar;
    CartesianSpeakerPosition cartesian;
  };
  struct ChannelFrequency {
    Optional<double> lowPass;
    Optional<double> highPass;
  };
  struct DirectSpeakersTypeMetadata {
    /// the `speakerLabel` tags of the audioBlockFormat, in AXML order
    std::vector<std::string> speakerLabels = {};
    SpeakerPosition position = PolarSpeakerPosition();
    ChannelFrequency channelFrequency = {};
    /// of the audioPackFormat that references this channel directly, e.g. `AP_00010002`
    Optional<std::string> audioPackFormatID;
  };

  // typeDefinition == Objects

  /// libear: boost::variant<CartesianPosition, PolarPosition> (common_types.hpp:26)
  struct Position {
    Position(PolarPosition p = PolarPosition()) : isCartesian(false), polar(p) {}
    Position(CartesianPosition c) : isCartesian(true), cartesian(c) {}
    bool isCartesian;
    PolarPosition polar;
    CartesianPosition cartesian;
  };
  struct ChannelLock {
    ChannelLock(bool flag = false) : flag(flag) {}
    /// (libear: boost::optional<double> maxDistance)
    ChannelLock(bool flag, double maxDistance) : flag(flag), hasMaxDistance(true), maxDistance(maxDistance) {}
    bool flag;
    bool hasMaxDistance = false;
    double maxDistance = 0.0;
  };
  struct PolarObjectDivergence {
    PolarObjectDivergence(double divergence = 0.0, double azimuthRange = 45.0)
        : divergence(divergence), azimuthRange(azimuthRange) {}
    double divergence;
    double azimuthRange;
  };
  struct CartesianObjectDivergence {
    CartesianObjectDivergence(double divergence = 0.0, double positionRange = 0.0)
        : divergence(divergence), positionRange(positionRange) {}
    double divergence;
    double positionRange;
  };
  /// libear: boost::variant<PolarObjectDivergence, CartesianObjectDivergence>; the calculators only read
  /// `divergence` (and refuse anything but 0)
  struct ObjectDivergence {
    ObjectDivergence(double divergence = 0.0, double range = 45.0) : divergence(divergence), range(range) {}
    ObjectDivergence(PolarObjectDivergence d) : divergence(d.divergence), range(d.azimuthRange) {}
    ObjectDivergence(CartesianObjectDivergence d) : isCartesian(true), divergence(d.divergence), range(d.positionRange) {}
    bool isCartesian = false;
    double divergence, range;
  };
  struct PolarExclusionZone {
    float minAzimuth;
    float maxAzimuth;
    float minElevation;
    float maxElevation;
    float minDistance;
    float maxDistance;
    std::string label;
  };
  struct CartesianExclusionZone {
    float minX;
    float maxX;
    float minY;
    float maxY;
    float minZ;
    float maxZ;
    std::string label;
  };
  /// libear: boost::variant<PolarExclusionZone, CartesianExclusionZone>
  struct ExclusionZone {
    ExclusionZone() = default;
    ExclusionZone(PolarExclusionZone z) : isCartesian(false), polar(std::move(z)) {}
    ExclusionZone(CartesianExclusionZone z) : isCartesian(true), cartesian(std::move(z)) {}
    bool isCartesian = false;
    PolarExclusionZone polar = {};
    CartesianExclusionZone cartesian = {};
  };
  struct ZoneExclusion {
    std::vector<ExclusionZone> zones;
  };
  struct ObjectsTypeMetadata {
    Position position = {};
    double width = 0.0;
    double height = 0.0;
    double depth = 0.0;
    bool cartesian = false;
    double gain = 1.0;
    double diffuse = 0.0;
    ChannelLock channelLock = {};
    ObjectDivergence objectDivergence = {};
    ZoneExclusion zoneExclusion = {};
    bool screenRef = false;  ///< refused when set, as in libear
    Screen referenceScreen = getDefaultScreen();
  };

  struct HOATypeMetadata {
    std::vector<int> orders;
    std::vector<int> degrees;
    std::string normalization = std::string("SN3D");
    double nfcRefDist = 0.0;  ///< ignored, as in libear (which warns)
    bool screenRef = false;   ///< ignored, as in libear (which warns)
    Screen referenceScreen = getDefaultScreen();
  };
}  // namespace ear
