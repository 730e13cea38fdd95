// The host half of the overlay export (js/overlay-export.js re-exports it): the ITCZ line of the reference's pressure views
// (js/planet-mesh.js:1498-1538) and its latitude / longitude grids (buildGlobeGrid :427-469, buildMapGrid :385-412), as the
// Float32Arrays the reference hands to three.js, bit for bit.  It loads no native code, and
// planet_heightmap_generation_amd/overlay_export.py states the same functions byte for byte alike (V8's sin and cos there through
// wo_v8_math).  The map form of the ITCZ line does not subtract the centre meridian: the reference's behaviour, kept.

// ---- the ITCZ line -----------------------------------------------------------------------------------------------------------
// itczLine(itczLons, itczLats) -> { globe, map }: Float32Array positions, six per segment.  The globe polyline closes; the map form
// leaves out the segment across the antimeridian.
export function itczLine(itczLons, itczLats) {
    if (!(itczLons instanceof Float32Array) || !(itczLats instanceof Float32Array)) throw new TypeError('itczLine: itczLons and itczLats must be Float32Arrays');
    if (itczLons.length !== itczLats.length) throw new RangeError(`itczLons has ${itczLons.length} values and itczLats ${itczLats.length}`);
    const N = itczLons.length, R = 1.01, sx = 2 / Math.PI;
    const gPos = [], mPos = [];
    for (let i = 0; i < N; i++) {
        const j = (i + 1) % N;
        const lon0 = itczLons[i], lat0 = itczLats[i], lon1 = itczLons[j], lat1 = itczLats[j];
        const cosLat0 = Math.cos(lat0), cosLat1 = Math.cos(lat1);
        gPos.push(Math.sin(lon0) * cosLat0 * R, Math.sin(lat0) * R, Math.cos(lon0) * cosLat0 * R,
                  Math.sin(lon1) * cosLat1 * R, Math.sin(lat1) * R, Math.cos(lon1) * cosLat1 * R);
        const mx0 = lon0 * sx, my0 = lat0 * sx, mx1 = lon1 * sx, my1 = lat1 * sx;
        if (Math.abs(mx1 - mx0) > 1) continue;
        mPos.push(mx0, my0, 0.003, mx1, my1, 0.003);
    }
    return { globe: new Float32Array(gPos), map: new Float32Array(mPos) };
}

// ---- the grids ---------------------------------------------------------------------------------------------------------------
function checkSpacing(spacing) {
    const s = Number(spacing);
    if (!(Number.isFinite(s) && s > 0) || 360 / s > 100000) throw new RangeError(`the grid spacing is ${spacing} degrees: it must be a positive number that gives at most 100000 lines`);
    return s;
}
// globeGrid(spacing in degrees) -> Float32Array: circles of latitude (the poles left out), then meridians, 120 segments each, at radius 1.002
export function globeGrid(spacing) {
    spacing = checkSpacing(spacing);
    const R = 1.002, SEG = 120, positions = [];
    for (let deg = -90; deg <= 90; deg += spacing) {
        if (deg === -90 || deg === 90) continue;
        const lat = deg * Math.PI / 180, cosLat = Math.cos(lat), y = Math.sin(lat) * R;
        for (let i = 0; i < SEG; i++) {
            const lon0 = (i / SEG) * Math.PI * 2, lon1 = ((i + 1) / SEG) * Math.PI * 2;
            positions.push(Math.sin(lon0) * cosLat * R, y, Math.cos(lon0) * cosLat * R, Math.sin(lon1) * cosLat * R, y, Math.cos(lon1) * cosLat * R);
        }
    }
    for (let deg = -180; deg < 180; deg += spacing) {
        const lon = deg * Math.PI / 180, sinLon = Math.sin(lon), cosLon = Math.cos(lon);
        for (let i = 0; i < SEG; i++) {
            const lat0 = -Math.PI / 2 + (i / SEG) * Math.PI, lat1 = -Math.PI / 2 + ((i + 1) / SEG) * Math.PI;
            positions.push(sinLon * Math.cos(lat0) * R, Math.sin(lat0) * R, cosLon * Math.cos(lat0) * R, sinLon * Math.cos(lat1) * R, Math.sin(lat1) * R, cosLon * Math.cos(lat1) * R);
        }
    }
    return new Float32Array(positions);
}
// mapGrid(spacing in degrees, centerLon = 0) -> Float32Array: parallels, then meridians around the centre meridian, at z = 0.001
export function mapGrid(spacing, centerLon) {
    spacing = checkSpacing(spacing);
    const sx = 2 / Math.PI, Z = 0.001, PI = Math.PI, positions = [];
    const centerLonDeg = (Number(centerLon) || 0) * 180 / PI;
    for (let deg = -90; deg <= 90; deg += spacing) {
        const y = (deg * Math.PI / 180) * sx;
        positions.push(-2, y, Z, 2, y, Z);
    }
    for (let deg = -180; deg <= 180; deg += spacing) {
        let offsetDeg = deg - centerLonDeg;
        if (offsetDeg > 180) offsetDeg -= 360;
        else if (offsetDeg < -180) offsetDeg += 360;
        const x = (offsetDeg * Math.PI / 180) * sx;
        positions.push(x, -1, Z, x, 1, Z);
    }
    return new Float32Array(positions);
}
export function grids(spacing, centerLon) { return { globe: globeGrid(spacing), map: mapGrid(spacing, centerLon) }; }
