slope 1.3 1.25 1.1
offset -0.08 0.0 0.05
power 0.8 1.0 1.2
