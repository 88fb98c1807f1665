<?xml version="1.0" encoding="UTF-8"?>
<ColorCorrection id="bad_slope">
  <SOPNode>
    <Slope>1.3 1.25</Slope>
    <Offset>0 0 0</Offset>
    <Power>1 1 1</Power>
  </SOPNode>
</ColorCorrection>
