// Functional stand-in for grid_map::GridMap as the reference's GroundSegmentation translation unit uses it (TEST INFRASTRUCTURE).
// What it is: our own text; layers by name, the geometry, getIndex / isInside / setGeometry following grid_map_core 1.6.x as this
// project restates it (the same convention as ggo_get_index, written again here; no object code is shared).  What it is not:
// grid_map_core.  It has no move(), no start index other than (0, 0), no iterators, and it pins nothing about the real library.
#pragma once

#include <Eigen/Core>
#include <emmintrin.h>

#include <cmath>
#include <string>
#include <unordered_map>
#include <vector>

namespace grid_map {

typedef Eigen::MatrixXf Matrix;
typedef Eigen::Vector2d Position;
typedef Eigen::Vector2d Vector;
typedef Eigen::Array2d Length;
typedef Eigen::Array2i Index;
typedef Eigen::Array2i Size;

class GridMap {
public:
    GridMap() : size_(0, 0), resolution_(0.0), length_(0.0, 0.0), position_(0.0, 0.0) {}
    explicit GridMap(const std::vector<std::string>& layers) : GridMap()
    {
        for (const auto& l : layers) data_.insert({l, Matrix()});
    }
    void setFrameId(const std::string& id) { frame_ = id; }

    // size = round(length / resolution) per axis, every layer resized and cleared to NaN, length = size * resolution
    void setGeometry(const Length& length, const double resolution, const Position& position = Position(0.0, 0.0))
    {
        size_(0) = static_cast<int>(std::round(length(0) / resolution));
        size_(1) = static_cast<int>(std::round(length(1) / resolution));
        for (auto& kv : data_) {
            kv.second.resize(size_(0), size_(1));
            kv.second.setConstant(NAN);
        }
        resolution_ = resolution;
        length_(0) = static_cast<double>(size_(0)) * resolution_;
        length_(1) = static_cast<double>(size_(1)) * resolution_;
        position_ = position;
    }

    // an existing layer is assigned in place: references to it stay valid
    void add(const std::string& layer, const double value = NAN) { add(layer, Matrix::Constant(size_(0), size_(1), value)); }
    void add(const std::string& layer, const Matrix& data)
    {
        auto it = data_.find(layer);
        if (it != data_.end())
            it->second = data;
        else
            data_.insert({layer, data});
    }
    bool exists(const std::string& layer) const { return data_.count(layer) != 0; }
    Matrix& operator[](const std::string& layer) { return data_.at(layer); }
    const Matrix& operator[](const std::string& layer) const { return data_.at(layer); }

    const Size& getSize() const { return size_; }
    double getResolution() const { return resolution_; }
    const Length& getLength() const { return length_; }
    const Position& getPosition() const { return position_; }

    // getIndexFromPosition: ((position - 0.5 * length) - mapPosition) / resolution per axis, negated (map frame -> buffer order),
    // converted to int the way x86-64 converts (cvttsd2si: truncation, INT_MIN for NaN and out-of-range values)
    bool getIndex(const Position& position, Index& index) const
    {
        for (int a = 0; a < 2; ++a) {
            const double offset = 0.5 * length_(a);
            const double indexVector = ((position(a) - offset) - position_(a)) / resolution_;
            index(a) = _mm_cvttsd_si32(_mm_set_sd(-indexVector));
        }
        return isInside(position);
    }

    // checkIfPositionWithinMap: t = -Identity * ((position - mapPosition) - 0.5 * length), 0 <= t < length per axis
    bool isInside(const Position& position) const
    {
        const double ax = (position(0) - position_(0)) - 0.5 * length_(0);
        const double ay = (position(1) - position_(1)) - 0.5 * length_(1);
        const double tx = -1.0 * ax + 0.0 * ay;
        const double ty = 0.0 * ax + -1.0 * ay;
        return tx >= 0.0 && ty >= 0.0 && tx < length_(0) && ty < length_(1);
    }

private:
    std::unordered_map<std::string, Matrix> data_;
    Size size_;
    double resolution_;
    Length length_;
    Position position_;
    std::string frame_;
};

} // namespace grid_map
